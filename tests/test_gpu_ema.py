"""GPU: the weight average (EMA) kept by the fused Adam update.  The EMA variant of the kernel leaves Adam bitwise untouched; the average
follows its recurrence within rounding; swapped_ema() exchanges parameters, average and shadows in place and back; a replayed train step
with the average on matches one without it bitwise, also around an evaluation inside swapped_ema(); train -> checkpoint -> infer eval
--ema equals an evaluation of a model whose parameters were set from ema.* by hand."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 64


class Odd(torch.nn.Module):
    """Odd-sized parameters, a 3-element tail, more than one 256-byte bucket."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for i, shape in enumerate([(7, 13), (13,), (13, 5), (5,), (33, 3), (1,), (129,), (3,)]):
            setattr(self, f"w{i}", torch.nn.Parameter(torch.randn(shape, generator=g)))


def _grads(model, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(p.shape, generator=g) * scale for n, p in model.named_parameters()}


def _live(opt, t):
    return torch.cat([t[o:o + p.numel()] for p, o in zip(opt.params, opt.offsets)])


def test_ema_variant_leaves_adam_bitwise_untouched(dev):
    from video_vae_amd import optim
    sched = optim.warmup_cosine_decay_schedule(0.0, 1e-2, 3, 100, 1e-3)
    ma, mb = Odd(1).to(dev), Odd(1).to(dev)
    plain = optim.Optimizer(ma, sched, bucket_bytes=256)
    ema = optim.Optimizer(mb, sched, bucket_bytes=256, ema_decay=0.9)
    assert len(plain.buckets) > 1 and any(p.numel() % 4 for p in plain.params) and plain.params[0].numel() % 4 == 3
    assert torch.equal(ema.ema, ema.p)
    for step in range(8):
        gr = _grads(ma, 10 + step, 10.0 if step % 2 else 1e-2)           # the clip bites on every other step
        plain.set_grads(gr)
        ema.set_grads(gr)
        assert plain.update() == ema.update()
        for name in ("p", "m", "v", "shadow", "gnorm_sq", "g"):
            assert torch.equal(getattr(plain, name), getattr(ema, name)), (step, name)
        assert (plain.grad_norm() >= 1.0) == bool(step % 2)
    assert not torch.equal(_live(ema, ema.ema), _live(ema, ema.p))


def test_abi_argument_checks_and_odd_lengths(dev):
    """The Adam entry with an average, and the swap, on raw buffers: bad arguments are refused (a decay without an average among them); a
    length that is no multiple of 4 and operands that are not 16-byte aligned (the scalar variant of the swap) are handled to the last
    element and not one beyond."""
    from video_vae_amd._lib import lib
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 4099
    g = torch.Generator().manual_seed(0)
    mk = lambda: torch.randn(n + 8, generator=g).to(dev)
    p, gr, m, v, e = mk(), mk(), torch.zeros(n + 8, device=dev), torch.zeros(n + 8, device=dev), mk()
    sh = torch.zeros(n + 8, dtype=torch.bfloat16, device=dev)
    adam = lambda ema, d, cnt=1: lib().vvae_adam_clip_step(vp(p), vp(gr), None, vp(m), vp(v), vp(sh), n, None, 0, None, 1.0, 1.0, 1e-3, 0.9, 0.999,
                                                           1e-8, cnt, vp(ema), d, s)
    before = [t.clone() for t in (p, m, v, e)]
    for ema_arg, d in ((None, 0.9), (e, 1.0), (e, -0.1), (e, 1.5), (e, float("nan"))):
        assert adam(ema_arg, d) == 1001
    assert adam(e, 0.9, cnt=0) == 1001
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v, e)))      # a refused call launches nothing
    p0, e0 = p.clone(), e.clone()
    assert adam(e, 0.0) == 0                                                  # d = 0: the average is the new parameter
    torch.cuda.synchronize()
    assert torch.equal(e[:n], p[:n]) and torch.equal(e[n:], e0[n:]) and torch.equal(p[n:], p0[n:]) and not torch.equal(p[:n], p0[:n])
    assert torch.equal(sh[:n], p[:n].bfloat16()) and float(sh[n:].abs().max()) == 0
    swap = lib().vvae_swap_refresh_f32
    assert swap(None, vp(e), None, n, s) == 1001 and swap(vp(p), None, None, n, s) == 1001
    assert swap(vp(p), vp(p), None, n, s) == 1001 and swap(vp(p), vp(e), None, 0, s) == 1001
    for off in (0, 1):                                                       # 16-byte aligned quads + tail; 4-byte aligned scalars
        for with_bf16 in (True, False):
            a, b = mk(), mk()
            a0, b0 = a.clone(), b.clone()
            h = torch.zeros(n + 8, dtype=torch.bfloat16, device=dev)
            assert swap(vp(a[off:]), vp(b[off:]), vp(h[off:]) if with_bf16 else None, n, s) == 0
            torch.cuda.synchronize()
            assert torch.equal(a[off:off + n], b0[off:off + n]) and torch.equal(b[off:off + n], a0[off:off + n])
            assert torch.equal(a[:off], a0[:off]) and torch.equal(a[off + n:], a0[off + n:])
            assert torch.equal(b[:off], b0[:off]) and torch.equal(b[off + n:], b0[off + n:])
            if with_bf16:
                assert torch.equal(h[off:off + n], b0[off:off + n].bfloat16())
                assert float(h[:off].abs().sum()) == 0 and float(h[off + n:].abs().max()) == 0


def _check_recurrence(e_ref, big, ema_gpu, steps):
    """|ema - e| <= N 2^-22 M elementwise: per step at most two roundings of values no larger than M (one if the compiler contracts the
    sum to an fma), M the largest |p| or |e| the element has seen; the damping of old errors by d is not credited."""
    err = (ema_gpu.double().cpu() - e_ref).abs()
    bound = steps * 2.0 ** -22 * big
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("decay,warmup", [(0.9, False), (0.999, True)], ids=["constant", "warmup"])
def test_average_follows_the_recurrence(dev, decay, warmup):
    from video_vae_amd import optim
    m = Odd(2).to(dev)
    opt = optim.Optimizer(m, 1e-2, bucket_bytes=256, ema_decay=decay, ema_warmup=warmup)
    e = opt.p.double().cpu()
    big = e.abs()
    steps = 20
    for step in range(steps):
        opt.set_grads(_grads(m, 50 + step, 1.0))
        d_host = optim.ema_decay_at(decay, opt.count, warmup)
        opt.update()
        assert opt.last_ema_decay == d_host
        d = float(np.float32(d_host))                                        # the float32 value the kernel was handed
        p = opt.p.double().cpu()
        e = d * e + (1.0 - d) * p
        big = torch.maximum(big, torch.maximum(p.abs(), e.abs()))
    if warmup:
        assert d_host == 20 / 29 and opt.count == steps
    _check_recurrence(e, big, opt.ema, steps)
    assert float((opt.ema.double().cpu() - opt.p.double().cpu()).abs().max()) > 1e-3       # the average is not the iterate


def _small(flavour, seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def test_swapped_ema_exchanges_in_place_and_back(dev):
    from video_vae_amd import optim
    m = _small("model", 4).to(dev)
    opt = optim.Optimizer(m, 1e-3, ema_decay=0.5)
    assert opt.tpairs, "the small model has Linear kernels with transposed shadows"
    for _ in range(2):                                                       # two real updates on random gradients
        opt.g.normal_()
        opt.update()
    p_old, e_old, sh_old = opt.p.clone(), opt.ema.clone(), opt.shadow.clone()
    t_old = [t.clone() for _, t in opt.tpairs]
    assert not torch.equal(p_old, e_old)
    ptrs = lambda: [(p.data_ptr(), p.bf16.data_ptr(), p.ema.data_ptr(), p.bf16_t.data_ptr() if hasattr(p, "bf16_t") else 0) for p in opt.params]
    before = ptrs()
    with opt.swapped_ema() as inside:
        assert inside is opt and opt.ema_swapped
        assert torch.equal(opt.p, e_old) and torch.equal(opt.ema, p_old)
        assert torch.equal(opt.shadow, e_old.bfloat16())
        for p, o in zip(opt.params, opt.offsets):
            assert torch.equal(p.data.reshape(-1), e_old[o:o + p.numel()]) and torch.equal(p.bf16, p.data.bfloat16())
            if hasattr(p, "bf16_t"):
                assert torch.equal(p.bf16_t, p.bf16.t())
        assert ptrs() == before
        with pytest.raises(RuntimeError):
            opt.update()
    assert not opt.ema_swapped and ptrs() == before
    assert torch.equal(opt.p, p_old) and torch.equal(opt.ema, e_old) and torch.equal(opt.shadow, sh_old)
    for (_, t), want in zip(opt.tpairs, t_old):
        assert torch.equal(t, want)


def test_replayed_step_with_and_without_the_average(dev):
    """A GraphedTrainStep driven by an EMA optimizer against one driven by a plain optimizer: bitwise-equal parameters after every replay,
    the average on its recurrence (the capture's trial updates leave it where it was), and an evaluation inside swapped_ema() between
    two replays does not disturb the next one."""
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim
    from video_vae_amd.graph import GraphedTrainStep
    hw = (SMALL // 16) ** 2
    g = torch.Generator().manual_seed(5)
    videos = [torch.rand((2, 8, SMALL, SMALL, 3), generator=g).to(dev).to(torch.bfloat16) for _ in range(5)]
    mask = torch.ones((2, 8))
    mask[1, 6:] = 0
    mask = mask.to(dev)
    steps = {}
    for kind in ("plain", "ema"):
        m = _small("rl", 6).to(dev)
        opt = optim.Optimizer(m, 1e-3, **(dict(ema_decay=0.9) if kind == "ema" else {}))
        steps[kind] = (m, opt, GraphedTrainStep(m, opt, videos[0], mask, dict(L.HPARAMS), hw, V.Rngs(7), warmup=1))
    (mp_, plain, step_p), (me, ema, step_e) = steps["plain"], steps["ema"]
    assert torch.equal(plain.p, ema.p) and ema.count == 0
    assert torch.equal(ema.ema, ema.p)                                       # the capture's own updates did not leak into the average
    e = ema.p.double().cpu()
    big = e.abs()
    d = float(np.float32(0.9))
    for i, video in enumerate(videos):
        lp, _ = step_p(video, mask)
        le, _ = step_e(video, mask)
        assert torch.equal(lp, le), i
        assert torch.equal(plain.p, ema.p) and torch.equal(plain.m, ema.m) and torch.equal(plain.v, ema.v), i
        assert torch.equal(plain.shadow, ema.shadow), i
        p = ema.p.double().cpu()
        e = d * e + (1.0 - d) * p
        big = torch.maximum(big, torch.maximum(p.abs(), e.abs()))
        if i == 2:                                                           # evaluate the averaged weights between two replays
            with torch.no_grad():
                raw_loss = L.eval_step(me, video, mask, dict(L.HPARAMS), hw, V.Rngs(11))[0]
                with ema.swapped_ema():
                    ema_loss = L.eval_step(me, video, mask, dict(L.HPARAMS), hw, V.Rngs(11))[0]
            assert torch.isfinite(ema_loss) and float(ema_loss) != float(raw_loss)
            assert torch.equal(plain.p, ema.p)
    assert ema.count == len(videos)
    _check_recurrence(e, big, ema.ema, len(videos))
    assert not torch.equal(ema.ema, ema.p)


def _run(cmd, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_train_driver_keeps_saves_and_evaluates_the_average(dev, tmp_path):
    """python -m video_vae_amd.train --ema: the checkpoint carries ema.* next to the Adam state, --eval-ema evaluates inside swapped_ema()
    and says so; without --ema the validation line and the checkpoint's keys are what they were."""
    common = ["video_vae_amd.train", "--small", "--size", "32", "--per_device_batch_size", "2", "--max_frames", "8", "--steps", "5", "--log_every", "2",
              "--eval_steps", "1"]
    out = _run(common + ["--ema", "0.9", "--ema-warmup", "--eval-ema", "--save_dir", str(tmp_path / "a")], 300)
    val = [l for l in out.splitlines() if l.startswith("VALIDATION")]
    assert len(val) == 1 and "weights = ema" in val[0] and "nan" not in val[0].lower()
    assert any("mode = hipgraph" in l for l in out.splitlines())
    state = torch.load(tmp_path / "a" / "checkpoint_0" / "checkpoint.pt", weights_only=True)
    opt = state["optimizer"]
    assert opt["count"] == 5 and opt["ema_decay"] == 0.9
    names = [k[3:] for k in opt if k.startswith("mu.")]
    assert names and all(f"ema.{n}" in opt and opt[f"ema.{n}"].shape == state["model"][n].shape for n in names)
    assert any(not torch.equal(opt[f"ema.{n}"], state["model"][n]) for n in names)
    out = _run(common + ["--save_dir", str(tmp_path / "b")], 300)
    val = [l for l in out.splitlines() if l.startswith("VALIDATION")]
    assert len(val) == 1 and "weights" not in val[0]
    plain = torch.load(tmp_path / "b" / "checkpoint_0" / "checkpoint.pt", weights_only=True)["optimizer"]
    assert set(plain) == {"count"} | {f"{k}.{n}" for k in ("mu", "nu") for n in names}


def test_train_checkpoint_infer_eval_ema_end_to_end(dev, tmp_path):
    """The train driver's step runner (eager once, then one replayed graph) with --ema 0.9's optimizer, saved; ``infer eval --ema`` then
    gives exactly the numbers of ``infer eval`` on a checkpoint whose parameters were set from ema.* by hand (same graph, same weights),
    other numbers than the raw weights, and the JSON says which weights it ran."""
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim, train
    hw = (SMALL // 16) ** 2
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):                   # the driver's rule: ONE non-default stream for the whole run
        model = _small("rl", 8).to(dev)
        opt = optim.Optimizer(model, 1e-3, ema_decay=0.9)                    # (the driver's own schedule starts at lr = 0)
        said = []
        runner = train.StepRunner(model, opt, hw, V.Rngs(3), use_graph=True, capture_after=1, log=said.append)
        hparams = dict(L.HPARAMS)
        for batch in train.synthetic_batches(2, 8, (SMALL, SMALL), 1, 6, dev):
            loss, _ = runner(batch["video"].to(torch.bfloat16), batch["mask"], hparams)
        assert runner.mode == "hipgraph" and opt.count == 6 and torch.isfinite(loss), said
        V.save_checkpoint(model, opt, str(tmp_path / "ck"))
        torch.cuda.synchronize()
    state = torch.load(tmp_path / "ck" / "checkpoint.pt", weights_only=True)
    by_hand = _small("rl", 8)
    V.load_checkpoint(by_hand, None, str(tmp_path / "ck"))
    own = dict(by_hand.named_parameters())
    with torch.no_grad():
        for k, v in state["optimizer"].items():
            if k.startswith("ema."):
                own[k[4:]].copy_(v)
    V.save_checkpoint(by_hand, None, str(tmp_path / "hand"))
    rng = np.random.default_rng(4)
    data = tmp_path / "data"
    data.mkdir()
    np.save(data / "long.npy", rng.integers(0, 256, size=(12, 40, 48, 3), dtype=np.uint8))
    np.save(data / "short.npy", rng.integers(0, 256, size=(5, 40, 48, 3), dtype=np.uint8))
    res = {}
    for tag, ck, extra in (("ema", "ck", ["--ema"]), ("raw", "ck", []), ("hand", "hand", [])):
        out = tmp_path / f"{tag}.json"
        _run(["video_vae_amd.infer", "eval", "--model_path", str(tmp_path / ck), "--data", str(data), "--size", str(SMALL), "--frames", "8",
              "--batch", "2", "--small", "--threshold", "--per-frame", "--out", str(out)] + extra, 180)
        res[tag] = json.loads(out.read_text())
    assert res["ema"]["config"]["weights"] == "ema" and res["raw"]["config"]["weights"] == "raw" and res["hand"]["config"]["weights"] == "raw"
    assert res["ema"]["dataset"] == res["hand"]["dataset"] and res["ema"]["clips"] == res["hand"]["clips"]       # exactly
    assert res["ema"]["dataset"]["frames"] == 17
    for k in ("psnr", "ssim", "mse"):
        assert res["ema"]["dataset"][k] != res["raw"]["dataset"][k], k
    bare = subprocess.run([sys.executable, "-m", "video_vae_amd.infer", "eval", "--model_path", str(tmp_path / "hand"), "--data", str(data), "--size",
                           str(SMALL), "--frames", "8", "--batch", "2", "--small", "--threshold", "--ema", "--out", str(tmp_path / "x.json")],
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=180)
    assert bare.returncode != 0 and "no weight average" in bare.stderr       # a checkpoint without an average is an error, not raw weights
