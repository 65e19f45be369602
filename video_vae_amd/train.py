#!/usr/bin/env python3
"""Training driver: counterpart of the reference's train/rl_nonadversarial.py `__main__` (:216-391) and of the multi-host
loop claude_distributed/distributed_train.py (:433-583), for one node of MI355X GPUs.

    python -m video_vae_amd.train --steps 100                               # 1 GPU, synthetic clips
    python -m video_vae_amd.train --steps 100 --grad-accum 4                # one update per 4 batches: effective batch 4 x per-device
    python -m video_vae_amd.train --data DIR --crop_size 512 --device-resize # the reference's 512-crop, 256-resize recipe, resized on the GPU
    python -m video_vae_amd.train --data Y4MDIR --crop_size 512 --device-yuv # .y4m clips: plane bytes to the GPU, convert + resize in one launch
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m video_vae_amd.train --steps 100

Same constants (rl_nonadversarial.py:36-57), model config (:234-236), optimizer (:241-253), hparams (:255-263), batch/frames
curriculum (:287-295) and log keys (:344-359).  Data: any iterable of {"video": float32 (B,T,H,W,3) in [0,1], "mask": float32
(B,T)} batches (the reference's dataloader contract, train/dataloader.py:387-390): ``--data DIR`` streams clips from DIR through
video_vae_amd/data.py (worker processes -> pinned uint8 batches -> H2D on a side stream, per-rank shuffle seed + rank); without
--data this driver feeds seeded synthetic clips.  ``--crop_size N`` crops N x N and resizes to --size (the reference crops 512 and resizes
to 256, train/dataloader.py crop_size=512, resize=RESIZE; the default N = --size crops at native resolution and resizes nothing);
``--device-resize`` moves that resize from the workers to one HIP launch behind the H2D copy, same values; ``--device-yuv`` (a folder of
.y4m clips) moves the colour conversion there too: the workers copy plane bytes and one launch converts, resizes and normalises, same
values (``--y4m-matrix``, ``--y4m-range``: how .y4m clips are read, in every mode).  One process per GPU; gradients are all-reduced over RCCL overlapped with backward (ddp.py); rank 0 logs;
SIGTERM/SIGINT flips a flag and the loop checkpoints and exits (distributed_train.py:58-67,489-494).

The step runs on the path bench.py measures: ``StepRunner`` keeps one captured ``GraphedTrainStep`` per (batch, frames) shape of the
curriculum -- the counterpart of the reference's ``nnx.jit(train_step)`` (rl_nonadversarial.py:276-277,332), which also compiles once
per shape -- and runs eagerly only until a shape has been seen ``--capture_after`` times (a shape met once is not worth a capture) or
with ``--eager``.  ``--grad-accum K`` sums the gradients of K consecutive batches (micro-steps) and applies one update with their mean
(optax.MultiSteps; optim.Optimizer(accum_steps=K)): the same captured graph serves every micro-step, ``--steps`` keeps counting batches,
the schedule is sized for the effective batch and a log line appears once per applied update.  Every ``--sample_every`` steps the
reconstruction and the original of one clip are written with data.batch_to_video
(rl_nonadversarial.py:337-343); after every epoch ``--eval_steps`` batches go through eval_step (:200-208,362-391).
"""
import argparse
import contextlib
import gc
import math
import os
import signal
import statistics
import time

import torch
import torch.distributed as dist

import video_vae_amd as V
from video_vae_amd import ddp, loss as L, optim, rl_model

NUM_EPOCHS, BATCH_SIZE, MAX_FRAMES, RESIZE, SEED = 100, 2, 32, (256, 256), 0
NEGATIVE_PENALTY_TRAINING_STEPS = 2000
_SHOULD_STOP = False
TIMES = []                    # (start event, end event, launch mode) per step, read after the loop


def _stop(signum, frame):
    global _SHOULD_STOP
    _SHOULD_STOP = True


def synthetic_batches(batch, frames, size, seed, steps, device, pool=4):
    """Seeded synthetic clips with ragged lengths: a pool of ``pool`` device-resident batches, cycled (generating 12.6 M uniform floats
    per step on the host costs more than the train step it would feed)."""
    g = torch.Generator().manual_seed(seed)
    made = []
    for _ in range(min(pool, steps)):
        video = torch.rand((batch, frames, size[0], size[1], 3), generator=g)
        lens = torch.randint(max(1, frames // 2), frames + 1, (batch,), generator=g)
        mask = (torch.arange(frames)[None, :] < lens[:, None]).float()
        made.append({"video": video.to(device), "mask": mask.to(device)})
    for i in range(steps):
        yield made[i % len(made)]


class StepRunner:
    """train_step(video, mask, hparams) -> (loss, aux), replayed from a captured hipGraph once a shape has been seen often enough.

    One graph per input shape; a change of ``hparams`` (the compression-rate switch at step 2000, :327-328) re-captures that shape's
    graph, since the loss constants are baked into the captured launches.  Each graph draws its noise from its own ``Rngs`` (a captured
    step pins the draws of ITS rngs to static buffers; the eager fallback keeps drawing from the driver's)."""

    def __init__(self, model, opt, hw, rngs, perceptual_loss_fn=None, vgg_params=None, use_graph=True, capture_after=1, log=None, enc_segments=3):
        self.model, self.opt, self.hw, self.rngs = model, opt, hw, rngs
        self.ploss, self.vgg_params = perceptual_loss_fn, vgg_params
        self.use_graph, self.capture_after, self.log = use_graph, capture_after, log or (lambda msg: None)
        self.graphs, self.seen = {}, {}
        self.enc_segments = enc_segments
        self.mode = "eager"

    def __call__(self, video, mask, hparams):
        shape = (tuple(video.shape), video.dtype)
        hkey = tuple(sorted(hparams.items()))
        hit = self.graphs.get(shape)
        if hit is not None and hit[0] == hkey:
            self.mode = "hipgraph"
            loss, aux = hit[1](video, mask)
            return loss, dict(aux)
        n = self.seen[shape] = self.seen.get(shape, 0) + 1
        if self.use_graph and n > self.capture_after:
            from .graph import GraphedTrainStep
            if hit is not None:                                  # same shape, new loss constants: drop the old graph and its pool first
                del self.graphs[shape], hit
                gc.collect()
                torch.cuda.empty_cache()
            try:
                t0 = time.perf_counter()
                gc.collect()                                     # no autograd graph of an eager step may outlive into the capture
                g = GraphedTrainStep(self.model, self.opt, video, mask, dict(hparams), self.hw, V.Rngs(1_000_003 * (self.rngs.seed + 1) + len(self.seen)),
                                     perceptual_loss_fn=self.ploss, vgg_params=self.vgg_params, stream=torch.cuda.current_stream(),
                                     enc_segments=self.enc_segments)
                self.graphs[shape] = (hkey, g)
                self.log(f"captured the train step for video {tuple(video.shape)} in {time.perf_counter() - t0:.1f} s "
                         f"({1 + len(g.graphs)} hipGraph{'s' if g.graphs else ''})")
                self.mode = "hipgraph"
                loss, aux = g(video, mask)
                return loss, dict(aux)
            except Exception as e:                               # capture is an optimisation, never a requirement
                self.log(f"hipGraph capture failed ({type(e).__name__}: {e}); this shape stays eager")
                self.seen[shape] = -(1 << 30)
        self.mode = "eager"
        loss, aux = L.train_step(self.model, self.opt, video, mask, hparams, self.hw, self.rngs, self.ploss, self.vgg_params)
        return loss, aux


def build_schedule(per_device_batch_size, world, grad_accum=1):
    """The reference's schedule for the batch one update sees: per-device batch x ranks x accumulated micro-steps."""
    return optim.reference_schedule(batch_size=per_device_batch_size * world * grad_accum)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps per epoch for synthetic data")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--per_device_batch_size", type=int, default=BATCH_SIZE)
    ap.add_argument("--max_frames", type=int, default=MAX_FRAMES)
    ap.add_argument("--size", type=int, default=RESIZE[0])
    ap.add_argument("--flavour", default="rl", choices=["rl", "model"])
    ap.add_argument("--model_path", type=str, default=None, help="checkpoint directory to resume from")
    ap.add_argument("--save_dir", type=str, default=None)
    ap.add_argument("--small", action="store_true", help="tiny model (depth 1) for smoke runs")
    ap.add_argument("--data", type=str, default=None, help="directory of clips (videos{i}/*.npy|npz|mp4...): the host input pipeline")
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--grad-dtype", default="f32", choices=["f32", "bf16"], help="dtype of the gradient all-reduce (ddp.GradReducer)")
    ap.add_argument("--enc-segments", type=int, default=3, help="data parallel: hipGraphs the encoder's backward is cut into (graph.py)")
    ap.add_argument("--eager", action="store_true", help="never capture: every step through the eager L.train_step")
    ap.add_argument("--capture_after", type=int, default=1, help="eager steps of a (batch, frames) shape before its step is captured as a hipGraph")
    ap.add_argument("--log_every", type=int, default=10)
    ap.add_argument("--sample_every", type=int, default=0,
                    help="every N steps write the reconstruction and the original of one clip under --sample_dir (rl_nonadversarial.py:337-343: 500)")
    ap.add_argument("--sample_dir", type=str, default=None)
    ap.add_argument("--sample_ext", default="npz", choices=["npz", "npy", "mp4"], help="mp4 needs ffmpeg on PATH (data.batch_to_video)")
    ap.add_argument("--eval_steps", type=int, default=0, help="batches per epoch through eval_step after the epoch's training (:362-391)")
    ap.add_argument("--eval_data", type=str, default=None, help="directory of evaluation clips (default: synthetic / --data)")
    ap.add_argument("--vgg", type=str, default=None,
                    help="perceptual loss (rl flavour; rl_nonadversarial.py:125,272-274): 'random' = randomly initialised VGG16 head, or the "
                         "path of an .npz / .pt with its six tensors (the ImageNet weights are a remote download in the reference)")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="keep an exponential moving average of the weights with this decay, advanced inside the fused Adam update and "
                         "saved with the checkpoint (infer ... --ema evaluates it); default: no average")
    ap.add_argument("--ema-warmup", dest="ema_warmup", action="store_true",
                    help="--ema: the decay of update n (0-based) is min(DECAY, (1 + n) / (10 + n))")
    ap.add_argument("--eval-ema", dest="eval_ema", action="store_true", help="--ema: --eval_steps evaluates the averaged weights")
    ap.add_argument("--grad-accum", dest="grad_accum", type=int, default=1, metavar="K",
                    help="sum the gradients of K consecutive batches in fp32 and apply one clip + Adam update with their mean; --steps still "
                         "counts batches, the schedule is built for per_device_batch_size * world * K; default 1: every batch updates")
    ap.add_argument("--crop_size", type=int, default=None, metavar="N",
                    help="--data / --eval_data: one random N x N crop per clip, resized to --size (the reference: 512 -> 256); "
                         "default: --size, a crop at native resolution and no resize")
    ap.add_argument("--device-resize", dest="device_resize", action="store_true",
                    help="--data: the workers stop after the crop and the GPU resizes, divides by 255 and casts in one launch "
                         "(csrc/resize.hip: the host path's values, bit for bit) instead of the host's interpolate")
    ap.add_argument("--device-yuv", dest="device_yuv", action="store_true",
                    help="--data, a folder of .y4m clips of one chroma form: the workers copy the crop's plane bytes and the GPU converts to "
                         "RGB, resizes, divides by 255 and casts in one launch (csrc/yuv_window.hip: the host path's values, bit for bit)")
    ap.add_argument("--y4m-matrix", dest="y4m_matrix", default="bt601", choices=["bt601", "bt709"],
                    help=".y4m clips: the matrix the planes are converted with (the container carries none)")
    ap.add_argument("--y4m-range", dest="y4m_range", default="header", choices=["header", "limited", "full"],
                    help=".y4m clips: the range of the planes; header = limited unless the file says XCOLORRANGE=FULL")
    ap.add_argument("--quantise-bits", dest="quantise_bits", type=int, default=None, choices=range(2, 9), metavar="N",
                    help="quantisation-aware training: the decoder is trained on the kept frames' latents quantised to N bits (2 .. 8), the "
                         "numbers `infer eval --quantise-bits N` feeds it, with a straight-through gradient; the lines gain code_entropy "
                         "(bits per code of the batch's pooled histogram).  Not stored in checkpoints: pass it again on resume")
    ap.add_argument("--quantise-after", dest="quantise_after", type=int, default=0, metavar="STEPS",
                    help="--quantise-bits: the quantiser switches on with the first batch after STEPS batches that starts an accumulation "
                         "cycle (default 0: from the start); the switch re-captures the step's graph")
    ap.add_argument("--rate-weight", dest="rate_weight", type=float, default=None, metavar="LAMBDA",
                    help="--quantise-bits: add LAMBDA x rate_bpp to the loss, the relaxed cost in bits per pixel of the kept frames' codes "
                         "under the batch's own histogram (ops.latent_rate); switches on with the quantiser; the lines gain rate_bpp.  Not "
                         "stored in checkpoints")
    ap.add_argument("--ssim-weight", dest="ssim_weight", type=float, default=None, metavar="W",
                    help="add W x (1 - ssim) to the loss: the mean SSIM of the valid frames' reconstructions against the clip (11-tap "
                         "Gaussian window, unclamped operands; ops.ssim_frames, forward and backward in HIP inside the captured step); the "
                         "lines gain ssim.  Needs a frame the kernel takes (--size >= 11 and 3 x --size <= 2048).  Not stored in "
                         "checkpoints: pass it again on resume.  Default and 0: no SSIM term")
    return ap


def parse_args(argv=None):
    """The parsed arguments, checked: everything wrong with them is an argparse error before a GPU is touched."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.crop_size is None:
        args.crop_size = args.size
    if args.crop_size < args.size:
        ap.error(f"--crop_size {args.crop_size} is below --size {args.size}: the crop is resized down to --size, never up")
    if args.device_resize and not args.data:
        ap.error("--device-resize needs --data: synthetic batches are made on the device at --size")
    if args.device_yuv and not args.data:
        ap.error("--device-yuv needs --data: a folder of .y4m clips")
    if args.ema is not None and not 0.0 <= args.ema < 1.0:
        ap.error("--ema DECAY is in [0, 1)")
    if (args.ema_warmup or args.eval_ema) and args.ema is None:
        ap.error("--ema-warmup and --eval-ema need --ema DECAY")
    if args.grad_accum < 1:
        ap.error("--grad-accum K is an integer >= 1")
    if args.quantise_after and args.quantise_bits is None:
        ap.error("--quantise-after needs --quantise-bits N")
    if args.rate_weight is not None and args.quantise_bits is None:
        ap.error("--rate-weight needs --quantise-bits N")
    if args.rate_weight is not None and not args.rate_weight >= 0:
        ap.error("--rate-weight LAMBDA is a number >= 0")
    if args.ssim_weight is not None and not args.ssim_weight >= 0:
        ap.error("--ssim-weight W is a number >= 0")
    if args.ssim_weight:
        from video_vae_amd import ops                             # a host-side question to the library: no GPU is touched
        if not ops.ssim_frames_supported(1, 1, args.size, args.size, 3):
            ap.error(f"--ssim-weight: frames of {args.size}x{args.size}x3 are outside what the SSIM kernels take ({ops.SSIM_LOSS_LIMITS})")
    if args.quantise_after < 0:
        ap.error("--quantise-after STEPS is an integer >= 0")
    if args.sample_every and not args.sample_dir:
        ap.error("--sample_every needs --sample_dir")
    return args


def data_batches(args, directory, bsz, frames, epoch, rank, dev):
    """Device batches of the clips under ``directory``: worker processes -> pinned uint8 -> H2D and conversion on a side stream."""
    from video_vae_amd import data as D
    size = (args.size, args.size)
    y4m = {"matrix": args.y4m_matrix, "range": args.y4m_range}
    yuv_kw = {}                                                   # only what differs from the defaults is passed down
    if args.device_yuv:
        yuv_kw["device_yuv"] = True
    if args.device_yuv or y4m != {"matrix": "bt601", "range": "header"}:
        yuv_kw["y4m"] = y4m
    host = D.create_batched_dataloader(directory, batch_size=bsz, max_frames=frames, resize=size, crop_size=args.crop_size,
                                       shuffle=True, seed=SEED + epoch, num_workers=args.num_workers, prefetch_size=16,
                                       drop_remainder=True, rank=rank, num_epochs=1, as_uint8=True, device_resize=args.device_resize,
                                       **yuv_kw)
    # the cast of :330 rides in the H2D side stream
    if args.device_yuv:
        return D.DevicePrefetcher(host, dev, dtype=torch.bfloat16, resize=size, yuv=dict(host.yuv))
    return D.DevicePrefetcher(host, dev, dtype=torch.bfloat16, resize=size if args.device_resize else None)


def main(argv=None):
    args = parse_args(argv)

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC for RCCL between the ranks; before the first GPU call
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # ONE non-default stream for the whole run: model construction, eager steps, graph captures and replays, the optimizer update and
    # (through the current-stream edges of ProcessGroupNCCL) the collectives.  Autograd pins every parameter's AccumulateGrad node to the
    # stream that was current when the node was made; a capture on another stream than the eager steps before it crashes the engine.
    train_stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(train_stream)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    signal.signal(signal.SIGTERM, _stop)
    signal.signal(signal.SIGINT, _stop)

    size, patch = args.size, 16
    hw = (size // patch) ** 2
    cfg = dict(height=size, width=size, channels=3, patch_size=patch, encoder_depth=9, decoder_depth=12, mlp_dim=1536,
               num_heads=8, qkv_features=512, max_temporal_len=64, spatial_compression_rate=8, unembedding_upsample_rate=4)
    if args.small:
        cfg.update(encoder_depth=1, decoder_depth=1, mlp_dim=256, qkv_features=128, num_heads=4)
    cls = rl_model.VideoVAE if args.flavour == "rl" else V.VideoVAE
    model = cls(rngs=V.Rngs(2), **cfg).to(dev)
    accum = args.grad_accum
    opt = optim.Optimizer(model, build_schedule(args.per_device_batch_size, world, accum), ema_decay=args.ema, ema_warmup=args.ema_warmup,
                          accum_steps=accum)
    red = ddp.GradReducer(opt, grad_dtype=torch.bfloat16 if args.grad_dtype == "bf16" else torch.float32) if world > 1 else None
    hparams = dict(L.HPARAMS)
    if args.ssim_weight:
        hparams["ssim_weight"] = args.ssim_weight                 # from the first step: the step is captured with the term (loss.add_ssim_term)
    if args.model_path:
        if rank == 0 or world == 1:
            V.load_checkpoint(model, opt, args.model_path)
        hparams["max_compression_rate"] = 100000                  # rl_nonadversarial.py:265-268
    if red is not None:
        # replicate rank 0's parameters, Adam moments and update count (start-up and resume: rank-0 restore + broadcast of
        # {"model", "optimizer"}, claude_distributed/distributed_train.py:321-341,378-380)
        red.broadcast_state(0)
    if rank == 0:
        print(f"Trainable Parameters: {sum(p.numel() for p in model.parameters()) / 1e6} Million", flush=True)

    ploss = vgg_params = None
    if args.vgg:
        from video_vae_amd import perceptual
        vgg, vgg_params = perceptual.load_vgg(None if args.vgg == "random" else args.vgg, device=dev)
        ploss = perceptual.get_adversarial_perceptual_loss_fn(vgg)
    rngs = V.Rngs(3 + rank)
    log = (lambda msg: print(msg, flush=True)) if rank == 0 else (lambda msg: None)
    runner = StepRunner(model, opt, hw, rngs, ploss, vgg_params, use_graph=not args.eager, capture_after=args.capture_after, log=log,
                        enc_segments=args.enc_segments)

    def loader(epoch, bsz, frames, directory, salt):
        if directory:
            return data_batches(args, directory, bsz, frames, epoch, rank, dev)
        return synthetic_batches(bsz, frames, (size, size), SEED + epoch + 1000 * rank + salt, max(args.steps, args.eval_steps), dev)

    def dump(tag, epoch, i, batch, recon, bsz):
        from video_vae_amd import data as D
        d = os.path.join(args.sample_dir, f"{tag}/epoch{epoch}")
        os.makedirs(d, exist_ok=True)
        D.batch_to_video({"video": recon[:bsz], "mask": batch["mask"]}, os.path.join(d, f"video_{i}_latent.{args.sample_ext}"), fps=30.0)
        D.batch_to_video(batch, os.path.join(d, f"video_{i}_original.{args.sample_ext}"), fps=30.0)

    start, global_step = time.perf_counter(), 0
    for epoch in range(args.epochs):
        max_mult = min(int(math.log2(max(args.per_device_batch_size, 1))), int(math.log2(64 / args.max_frames)) - 1)
        mult = max(0, min(epoch, max_mult))                       # batch <-> frames curriculum, :287-295
        bsz, frames = args.per_device_batch_size // (2 ** mult), args.max_frames * (2 ** mult)
        updates, cycle = 0, None                                  # applied updates of this epoch; device-side sums over the running cycle
        for i, batch in enumerate(loader(epoch, bsz, frames, args.data, 0)):
            if _SHOULD_STOP or i >= args.steps:
                break
            if i > NEGATIVE_PENALTY_TRAINING_STEPS:
                hparams["max_compression_rate"] = 10000
            if args.quantise_bits is not None and "quant_bits" not in hparams and global_step >= args.quantise_after and opt.micro == 0:
                hparams["quant_bits"] = args.quantise_bits        # from this cycle on the decoder sees quantised latents (loss.set_quantiser)
                if args.rate_weight:
                    hparams["rate_weight"] = args.rate_weight     # ... and the loss prices their codes
            video = batch["video"].to(torch.bfloat16)             # :330
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()                                           # step i = this event -> the next step's (bench.py's per-step clock)
            loss, aux = runner(video, batch["mask"], hparams)
            TIMES.append((ev, runner.mode))
            global_step += 1
            if args.sample_every and i % args.sample_every == args.sample_every - 1 and rank == 0:
                recon = aux.get("reconstruction")
                if recon is None:                                 # a replayed step keeps no reconstruction: one eval pass on this batch
                    recon = L.eval_step(model, video, batch["mask"], hparams, hw, rngs, ploss, vgg_params)[1]["reconstruction"]
                dump("train", epoch, i, batch, recon, bsz)
            if accum > 1:                                         # loss and aux of the cycle, summed on the device: no sync per micro-step
                keys = [k for k in aux if k != "reconstruction"]
                now = torch.stack([v.detach().float().reshape(()) for v in [loss] + [aux[k] for k in keys]])
                cycle = now if cycle is None else cycle + now
            if not opt.last_update:                               # a micro-step that only accumulated: lines are per applied update
                continue
            updates += 1
            if (updates - 1) % args.log_every == 0 or i + accum >= args.steps:
                keys = [k for k in aux if k != "reconstruction"]
                vals = [loss] + [aux[k] for k in keys] if accum == 1 else list((cycle / accum).unbind())
                if world > 1:
                    vals = ddp.all_reduce_mean_scalars(vals)
                if rank == 0:
                    msg = ", ".join(f"{k} = {float(v):.4f}" for k, v in zip(["Loss"] + keys, vals))
                    print(f"Epoch {epoch}, Step {i}: {msg}, lr = {opt.last_lr:.3e}, time = {time.perf_counter() - start:.2f}, "
                          f"mode = {runner.mode}, grad_accum = {accum}, effective_batch_size = {bsz * accum}, effective_max_frames = {frames}",
                          flush=True)
            cycle = None
        if opt.micro:                                             # the next epoch has another batch shape (and a checkpoint holds no accumulator):
            log(f"Epoch {epoch}: dropped a partial accumulation cycle of {opt.micro} of {accum} micro-steps")     # mixing them would mis-weight clips
            opt.reset_accumulation()
        if args.save_dir and rank == 0:
            tag = "checkpoint_sigterm" if _SHOULD_STOP else "checkpoint"
            V.save_checkpoint(model, opt, os.path.join(args.save_dir, f"{tag}_{epoch}"))
        if args.eval_steps and not _SHOULD_STOP:
            evaluated = f", weights = {'ema' if args.eval_ema else 'raw'}" if args.ema is not None else ""
            # --eval-ema: the average sits in the parameters' place for the whole evaluation (one swap in, one swap back)
            with opt.swapped_ema() if args.eval_ema else contextlib.nullcontext():
                for i, batch in enumerate(loader(epoch, bsz, frames, args.eval_data or args.data, 500_000)):
                    if _SHOULD_STOP or i >= args.eval_steps:
                        break
                    video = batch["video"].to(torch.bfloat16)
                    loss, aux = L.eval_step(model, video, batch["mask"], hparams, hw, rngs, ploss, vgg_params)
                    if args.sample_every and i % 100 == 0 and rank == 0:
                        dump("eval", epoch, i, batch, aux["reconstruction"], bsz)
                    keys = [k for k in aux if k != "reconstruction"]
                    vals = [loss] + [aux[k] for k in keys]
                    if world > 1:
                        vals = ddp.all_reduce_mean_scalars(vals)
                    if rank == 0:
                        msg = ", ".join(f"{k} = {float(v):.4f}" for k, v in zip(["Loss"] + keys, vals))
                        print(f"VALIDATION Epoch {epoch}, Step {i}: {msg}{evaluated}, effective_batch_size = {bsz}, "
                              f"effective_max_frames = {frames}", flush=True)
        if world > 1:
            dist.barrier()
        if _SHOULD_STOP:
            break
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    torch.cuda.synchronize()
    if rank == 0 and TIMES:
        by_mode = {}
        for (a, mode), (b, mode_next) in zip(TIMES, TIMES[1:] + [(end, None)]):
            if mode_next in (mode, None):                              # a step followed by a capture is not a steady-state step
                by_mode.setdefault(mode, []).append(a.elapsed_time(b))
        for mode, ts in by_mode.items():
            tail = ts[len(ts) // 5:] if len(ts) >= 10 else ts          # the first fifth carries clock ramp and allocator warm-up
            print(f"train summary: {len(ts)} {mode} steps, median {statistics.median(tail):.2f} ms/step over the last {len(tail)} "
                  f"(logging every {args.log_every} steps included)", flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
