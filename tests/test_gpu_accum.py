"""GPU: gradient accumulation in the optimizer tail (optim.Optimizer(accum_steps=K), optax.MultiSteps semantics).  K micro-steps summed in
fp32 in arrival order and ONE clip + Adam (+ weight average) update with their mean: bitwise against a plain optimizer fed that mean for
K a power of two, against the optax restatement for K = 3; the raw entries (fold, squared norm and Adam on g + acc); the train step on
the model; a hipGraph captured between two micro-steps of a cycle; the training driver's --grad-accum; two ranks on one GPU."""
import ctypes
import gc
import os
import socket
import subprocess
import sys

import pytest
import torch

from oracle import optim as OOpt
from util import assert_close, rnd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(height=32, width=32, channels=3, patch_size=8, encoder_depth=1, decoder_depth=1, mlp_dim=64, num_heads=4,
            qkv_features=32, max_temporal_len=8, spatial_compression_rate=4, unembedding_upsample_rate=4)


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


def _sum_in_order(gs):
    """((g1 + g2) + g3) + ... in fp32 on the host, per parameter."""
    out = {}
    for n in gs[0]:
        s = gs[0][n]
        for g in gs[1:]:
            s = s + g[n]
        out[n] = s
    return out


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("K", [2, 4])
def test_cycles_equal_a_plain_optimizer_fed_the_mean_bitwise(dev, K, ema):
    """K a power of two: 1/K, K^2 and the clip factor's scaling are exact, so accumulating K gradients and updating once equals, bit for
    bit, a plain optimizer that was handed ((g1 + g2) + ...) * (1/K).  The clip bites on every other cycle."""
    from video_vae_amd import optim
    sched = optim.warmup_cosine_decay_schedule(0.0, 1e-2, 3, 100, 1e-3)
    ma, mb = Odd(1).to(dev), Odd(1).to(dev)
    kw = dict(bucket_bytes=256, **(dict(ema_decay=0.9) if ema else {}))
    a = optim.Optimizer(ma, sched, accum_steps=K, **kw)
    b = optim.Optimizer(mb, sched, **kw)
    assert len(a.buckets) > 1 and any(p.numel() % 4 for p in a.params) and a.params[0].numel() % 4 == 3
    assert b.acc is None and a.acc.shape == a.g.shape
    state = ("p", "m", "v", "shadow") + (("ema",) if ema else ())
    for cycle in range(4):
        gs = [_grads(ma, 100 + cycle * K + k, 10.0 if cycle % 2 else 1e-2) for k in range(K)]
        before = {n: getattr(a, n).clone() for n in state}
        count = a.count
        for k, gr in enumerate(gs[:-1]):
            a.set_grads(gr)
            assert a.update() is None and a.last_update is False and a.micro == k + 1
            assert a.count == count and all(torch.equal(getattr(a, n), before[n]) for n in state), (cycle, k)
        a.set_grads(gs[-1])
        lr = a.update()
        assert a.last_update is True and a.micro == 0 and a.count == count + 1 and a.last_lr == lr
        b.set_grads({n: s * (1.0 / K) for n, s in _sum_in_order(gs).items()})
        assert b.update() == lr and b.count == a.count
        for n in state:
            assert torch.equal(getattr(a, n), getattr(b, n)), (cycle, n)
        assert float(a.gnorm_sq.item()) == K * K * float(b.gnorm_sq.item())
        assert a.grad_norm() == b.grad_norm() and (a.grad_norm() >= 1.0) == bool(cycle % 2)
        assert torch.equal(a.p, before["p"]) == (lr == 0.0)                  # (the schedule starts at 0: the first update moves m and v only)


def test_three_micro_steps_against_the_optax_restatement(dev):
    """K = 3 (1/3 is not exact: no bitwise twin): three cycles against oracle/optim.py fed the fp64 mean of each cycle's three gradients, at the
    tolerances tests/test_gpu_model.py::test_optimizer_steps_match_oracle uses for this kernel."""
    import video_vae_amd as V
    from video_vae_amd import optim
    m = V.UNet(4, 8, 1, 3, V.Rngs(1), dtype=torch.float32)
    p0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(dev)
    kw = dict(init_value=0.0, peak_value=1e-2, warmup_steps=2, decay_steps=10, end_value=1e-3)
    opt = optim.Optimizer(m, optim.warmup_cosine_decay_schedule(**kw), max_norm=1.0, accum_steps=3)
    adam = OOpt.Adam(p0)
    po = p0
    for cycle in range(3):
        gs = [{k: rnd(v.shape, 100 + (3 * cycle + j) * 31 + i, 0.3 if cycle else 5.0) for i, (k, v) in enumerate(p0.items())} for j in range(3)]
        for j, gr in enumerate(gs):
            opt.set_grads(gr)
            assert (opt.update() is None) == (j < 2)
        mean = {k: (gs[0][k].double() + gs[1][k].double() + gs[2][k].double()) / 3.0 for k in p0}
        po, gn, lr = OOpt.train_update(po, mean, adam, kw)
        assert opt.count == cycle + 1 and abs(opt.last_lr - lr) <= 1e-12
        assert abs(opt.grad_norm() - float(gn)) <= 1e-4 * float(gn)
        for k, prm in m.named_parameters():
            assert_close(prm, po[k], rtol=1e-4, atol=1e-6, what=f"cycle{cycle} {k}")


def test_abi_refusals_fold_alignments_and_zero_accumulator(dev):
    """The fold, norm and Adam entries on raw buffers.  Bad arguments return 1001 and launch nothing.  vvae_grad_fold_f32 at n = 4099 (quads
    + a 3-element tail), 16-byte aligned and not (the scalar variant), overwriting and adding: bitwise torch.add, the 8 elements on either
    side untouched.  With an all-zero accumulator the squared-norm and Adam entries reproduce acc = NULL bit for bit, and with a real one
    acc = NULL on torch's g + acc."""
    from video_vae_amd._lib import lib
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, G = 4099, 8
    gen = torch.Generator().manual_seed(0)
    mk = lambda k=n: torch.randn(k, generator=gen).to(dev)
    fold, sq = lib().vvae_grad_fold_f32, lib().vvae_sqnorm_partials
    # ---- refusals
    d, r = mk(), mk()
    nb = lib().vvae_sqnorm_blocks(n)
    part = torch.full((nb,), -1.0, dtype=torch.float64, device=dev)
    p, m, v, e = mk(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), mk()
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    adam_acc = lambda acc, ema, dec, cnt=1, pp=p, mm=m, vv=v, shh=sh, gp=None, nparts=0, out=None, g=r: lib().vvae_adam_clip_step(
        vp(pp), vp(g), vp(acc), vp(mm), vp(vv), vp(shh), n, vp(gp), nparts, vp(out), 1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, cnt, vp(ema), dec, s)
    odd = mk(n + 4)[1:]                                                        # 4 bytes past a 16-byte boundary
    assert d.data_ptr() % 16 == 0 and r.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 4
    keep = [t.clone() for t in (d, r, part, p, m, v, e, sh)]
    assert fold(None, vp(r), n, 0, s) == 1001 and fold(vp(d), None, n, 1, s) == 1001 and fold(vp(d), vp(d), n, 0, s) == 1001
    assert fold(vp(d), vp(r), 0, 0, s) == 1001 and fold(vp(d), vp(r), -4, 1, s) == 1001
    for a in (r, None):                                                        # with an accumulator and without
        assert sq(None, vp(a), n, vp(part), s) == 1001 and sq(vp(d), vp(a), n, None, s) == 1001
        assert sq(vp(d), vp(a), 0, vp(part), s) == 1001 and sq(vp(d), vp(a), -4, vp(part), s) == 1001
        assert sq(vp(odd), vp(a), n, vp(part), s) == 1001
        assert adam_acc(a, None, 0.0, cnt=0) == 1001 and adam_acc(a, None, 0.0, g=None) == 1001
        assert adam_acc(a, None, 0.0, pp=None) == 1001 and adam_acc(a, None, 0.0, mm=None) == 1001 and adam_acc(a, None, 0.0, vv=None) == 1001
    assert sq(vp(d), vp(odd), n, vp(part), s) == 1001                          # an accumulator that is not 16-byte aligned
    for dec in (1.0, -0.1, float("nan")):
        assert adam_acc(d, e, dec) == 1001
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(keep, (d, r, part, p, m, v, e, sh)))
    # ---- the fold: (dst offset, src offset) in elements past a 16-byte aligned start
    for od, os_ in ((0, 0), (1, 1), (0, 1)):
        for overwrite in (0, 1):
            dst, src = mk(n + 2 * G + 1), mk(n + 2 * G + 1)
            dst0 = dst.clone()
            lo, so = G + od, G + os_
            assert (dst[lo:].data_ptr() % 16 == 0) == (od == 0) and (src[so:].data_ptr() % 16 == 0) == (os_ == 0)
            assert fold(vp(dst[lo:]), vp(src[so:]), n, overwrite, s) == 0
            torch.cuda.synchronize()
            want = torch.add(torch.zeros(n, device=dev) if overwrite else dst0[lo:lo + n], src[so:so + n])
            assert torch.equal(dst[lo:lo + n], want), (od, os_, overwrite)
            assert torch.equal(dst[:lo], dst0[:lo]) and torch.equal(dst[lo + n:], dst0[lo + n:]), (od, os_, overwrite)
    # ---- g + 0 with the accumulator given = g with acc = NULL
    g, acc, zero = mk(), mk(), torch.zeros(n, device=dev)
    pa, pb = torch.zeros(nb, dtype=torch.float64, device=dev), torch.zeros(nb, dtype=torch.float64, device=dev)
    assert sq(vp(g), None, n, vp(pa), s) == 0 and sq(vp(g), vp(zero), n, vp(pb), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and float(pa.sum()) > 1.0                       # (the clip below bites)
    summed = torch.add(g, acc)
    pc, pd = torch.zeros_like(pa), torch.zeros_like(pa)
    assert sq(vp(summed), None, n, vp(pc), s) == 0 and sq(vp(g), vp(acc), n, vp(pd), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(pc, pd) and not torch.equal(pc, pa)
    for with_ema in (False, True):
        for acc_t, g_sum, parts in ((zero, g, pa), (acc, summed, pc)):           # acc = NULL on g (or on g + acc summed by torch) | acc given beside g
            runs = []
            for g_t, a_t in ((g_sum, None), (g, acc_t)):
                pp, mm, vv, ee = p.clone(), m.clone() + 0.5, v.clone() + 0.25, e.clone()
                shh, out = torch.zeros(n, dtype=torch.bfloat16, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
                code = adam_acc(a_t, ee if with_ema else None, 0.9 if with_ema else 0.0, cnt=3, pp=pp, mm=mm, vv=vv, shh=shh, gp=parts,
                                nparts=nb, out=out, g=g_t)
                assert code == 0
                torch.cuda.synchronize()
                runs.append((pp, mm, vv, ee, shh, out))
            for x, y in zip(*runs):
                assert torch.equal(x, y), (with_ema, acc_t is zero)
            assert not torch.equal(runs[0][0], p) and torch.equal(runs[0][3], e) != with_ema


def _flat_to_named(opt, flat):
    return {n: flat[o:o + p.numel()].view(p.shape).clone() for n, p, o in zip(opt.names, opt.params, opt.offsets)}


def test_two_train_steps_accumulate_into_one_update_on_the_model(dev):
    """The tiny rl VideoVAE, fp32: two L.train_step calls on two batches with accum_steps = 2 leave exactly the parameters of one plain
    update with (g1 + g2) * 0.5, g1 and g2 taken from a twin whose learning rate is zero (same weights, same Rngs seeds, same batches)."""
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim, rl_model
    gen = torch.Generator().manual_seed(7)
    videos = [torch.rand((2, 8, 32, 32, 3), generator=gen).to(dev) for _ in range(2)]
    mask = torch.ones(2, 8)
    mask[1, 6:] = 0
    mask = mask.to(dev)
    build = lambda: rl_model.VideoVAE(rngs=V.Rngs(2), dtype=torch.float32, **TINY).to(dev)
    ma, mt, mc = build(), build(), build()
    a = optim.Optimizer(ma, 1e-3, accum_steps=2)
    twin = optim.Optimizer(mt, 0.0)
    third = optim.Optimizer(mc, 1e-3)
    assert torch.equal(a.p, twin.p) and torch.equal(a.p, third.p)
    ra, rt = V.Rngs(3), V.Rngs(3)
    gs = []
    for i, video in enumerate(videos):
        L.train_step(ma, a, video, mask, L.HPARAMS, 16, ra)
        assert a.last_update == bool(i) and a.micro == 1 - i
        L.train_step(mt, twin, video, mask, L.HPARAMS, 16, rt)
        gs.append(twin.g.clone())
        assert torch.equal(twin.p, third.p)                                   # lr = 0: the twin's weights never move
    assert not torch.equal(gs[0], gs[1])
    third.set_grads(_flat_to_named(third, (gs[0] + gs[1]) * 0.5))
    third.update()
    assert a.count == 1 and third.count == 1
    assert torch.equal(a.p, third.p) and torch.equal(a.m, third.m) and torch.equal(a.v, third.v) and torch.equal(a.shadow, third.shadow)
    assert not torch.equal(a.p, twin.p)


def test_capture_between_two_micro_steps_leaves_the_cycle_alone(dev):
    """A shape is captured on its second occurrence, which may be the middle of a cycle: the capture's own passes and updates must put back
    the accumulator and the micro-step counter next to p, m, v and count; the first replay then completes the cycle."""
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim, rl_model
    from video_vae_amd.graph import GraphedTrainStep
    gen = torch.Generator().manual_seed(9)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):                    # the driver's rule: ONE non-default stream for the whole run
        videos = [torch.rand((2, 8, 32, 32, 3), generator=gen).to(dev).to(torch.bfloat16) for _ in range(2)]
        mask = torch.ones(2, 8, device=dev)
        m = rl_model.VideoVAE(rngs=V.Rngs(2), dtype=torch.bfloat16, **TINY).to(dev)
        opt = optim.Optimizer(m, 1e-3, accum_steps=2)
        L.train_step(m, opt, videos[0], mask, L.HPARAMS, 16, V.Rngs(3))
        assert opt.micro == 1 and opt.last_update is False and opt.count == 0
        gc.collect()
        before = [t.clone() for t in (opt.acc, opt.p, opt.m, opt.v)]
        assert float(_live(opt, opt.acc).abs().max()) > 0
        step = GraphedTrainStep(m, opt, videos[0], mask, L.HPARAMS, 16, V.Rngs(4), warmup=1, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert opt.micro == 1 and opt.count == 0 and opt.last_update is False
        for t, t0, name in zip((opt.acc, opt.p, opt.m, opt.v), before, ("acc", "p", "m", "v")):
            assert torch.equal(_live(opt, t), _live(opt, t0)), name
        loss, _ = step(videos[1], mask)
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and opt.last_update is True and opt.count == 1 and opt.micro == 0
        assert not torch.equal(opt.p, before[1]) and torch.isfinite(opt.p).all()
        assert step.census[0] is not None and all(c.get("memset", 0) == 0 and c.get("kernel", 0) > 50 for c in step.census), step.census
        step(videos[0], mask)                                                 # the next cycle's first micro-step: no update
        assert opt.last_update is False and opt.count == 1 and opt.micro == 1
        torch.cuda.synchronize()


def _train(args, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "video_vae_amd.train"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_train_driver_grad_accum(dev, tmp_path):
    """python -m video_vae_amd.train --grad-accum 2: --steps counts batches, a line per applied update carrying grad_accum and the effective
    batch, the saved update count is steps // 2; an odd --steps drops the partial cycle, says so, and saves the count of the full ones."""
    common = ["--small", "--size", "32", "--per_device_batch_size", "2", "--max_frames", "8", "--grad-accum", "2", "--log_every", "1"]
    out = _train(common + ["--steps", "6", "--save_dir", str(tmp_path / "a")])
    lines = [l for l in out.splitlines() if l.startswith("Epoch 0, Step")]
    assert len(lines) == 3 and all("grad_accum = 2, effective_batch_size = 4, effective_max_frames = 8" in l and "nan" not in l.lower() for l in lines), out[-3000:]
    assert [l.split(":")[0] for l in lines] == ["Epoch 0, Step 1", "Epoch 0, Step 3", "Epoch 0, Step 5"]
    assert "mode = hipgraph" in lines[-1] and "dropped a partial" not in out
    assert torch.load(tmp_path / "a" / "checkpoint_0" / "checkpoint.pt", weights_only=True)["optimizer"]["count"] == 3
    out = _train(common + ["--steps", "5", "--save_dir", str(tmp_path / "b")])
    assert sum(l.startswith("Epoch 0, Step") for l in out.splitlines()) == 2
    assert "Epoch 0: dropped a partial accumulation cycle of 1 of 2 micro-steps" in out
    assert torch.load(tmp_path / "b" / "checkpoint_0" / "checkpoint.pt", weights_only=True)["optimizer"]["count"] == 2


def _accum_ddp_worker(rank, world, port, out):
    """Two ranks sharing cuda:0 (gloo transport), K = 2: (a) explicit gradients through the landing path on the Odd module; (b) the staged
    hipGraph step of a VAE with three encoder blocks, whose buckets are prelaunched between the graphs on the last micro-step only."""
    import torch.distributed as dist
    import video_vae_amd as V
    from video_vae_amd import optim, ddp, loss as L
    from video_vae_amd.graph import GraphedTrainStep
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        res = {}
        m = Odd(1).to(dev)
        opt = optim.Optimizer(m, optim.warmup_cosine_decay_schedule(0.0, 1e-2, 3, 100, 1e-3), bucket_bytes=256, accum_steps=2)
        red = ddp.GradReducer(opt)
        calls = []
        launch = red.launch
        red.launch = lambda b: (calls.append(b), launch(b))[1]
        for cycle in range(2):
            for step in range(2):
                opt.set_grads(_grads(m, 1000 + 100 * cycle + 10 * rank + step, 10.0 if cycle else 1e-2))
                res[f"calls{cycle}{step}"] = len(calls)
                lr = opt.update()
                assert (lr is None) == (step == 0)
            res[f"gn{cycle}"] = opt.grad_norm()
        torch.cuda.synchronize()
        res.update(p=opt.p.cpu(), m=opt.m.cpu(), v=opt.v.cpu(), count=opt.count, nbuckets=len(opt.buckets))
        vae = V.VideoVAE(rngs=V.Rngs(2), dtype=torch.bfloat16, **dict(TINY, encoder_depth=3)).to(dev)
        vopt = optim.Optimizer(vae, 1e-3, bucket_bytes=64 << 10, accum_steps=2)
        vred = ddp.GradReducer(vopt)
        vred.broadcast_parameters(0)
        video = torch.rand((2, 8, 32, 32, 3), generator=torch.Generator().manual_seed(5 + rank)).to(dev, torch.bfloat16)
        mask = torch.ones(2, 8, device=dev)
        gstep = GraphedTrainStep(vae, vopt, video, mask, L.HPARAMS, 16, V.Rngs(3 + rank), warmup=1)
        vcalls = []
        vlaunch = vred.launch
        vred.launch = lambda b: (vcalls.append(b), vlaunch(b))[1]
        res["ngraphs"], res["vmicro0"], res["vcount0"] = 1 + len(gstep.graphs), vopt.micro, vopt.count
        p0 = vopt.p.clone()
        gstep()
        torch.cuda.synchronize()
        res["vcalls1"], res["vmoved1"] = len(vcalls), not torch.equal(vopt.p, p0)
        loss, _ = gstep()
        torch.cuda.synchronize()
        res.update(vcalls2=len(vcalls), vbuckets=len(vopt.buckets), vp=vopt.p.cpu(), vcount=vopt.count, vloss=float(loss),
                   vmoved2=not torch.equal(vopt.p, p0))
        torch.save(res, os.path.join(out, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_world2_sharing_one_gpu_accumulates_then_reduces(dev, tmp_path):
    """world_size 2 on the one GPU of the box, K = 2, two cycles (the clip bites on the second): nothing is communicated on a cycle's
    first micro-step, every bucket once on its second; both ranks end with bitwise equal parameters and moments, and these are BITWISE
    those of a single-process plain optimizer fed ((g_r0s1 + g_r0s2) + (g_r1s1 + g_r1s2)) * 0.25.  Bitwise equality is asserted because
    it holds by construction: each rank's fold is one fp32 add per element (g + acc, commutative), the all-reduce over two ranks is one more
    commutative add whichever rank's addend comes first, and the scalings by 1/4 are exact.  The staged hipGraph step (1 + 3 graphs)
    follows the same rule: no launch and no update on the first replay of a cycle, one launch per bucket and one update on the second."""
    import torch.multiprocessing as mp
    from video_vae_amd import optim
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_accum_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    nb = r0["nbuckets"]
    assert nb > 1 and r0["count"] == 2 and r1["count"] == 2
    for r in (r0, r1):
        assert [r[f"calls{c}{s}"] for c in range(2) for s in range(2)] == [0, nb, nb, 2 * nb]      # running totals, read between landing and update(): a cycle's second landing launches
    for k in ("p", "m", "v"):
        assert torch.equal(r0[k], r1[k]), k
    m = Odd(1).to(dev)
    plain = optim.Optimizer(m, optim.warmup_cosine_decay_schedule(0.0, 1e-2, 3, 100, 1e-3), bucket_bytes=256)
    for cycle in range(2):
        g = [[_grads(m, 1000 + 100 * cycle + 10 * rank + step, 10.0 if cycle else 1e-2) for step in range(2)] for rank in range(2)]
        plain.set_grads({n: ((g[0][0][n] + g[0][1][n]) + (g[1][0][n] + g[1][1][n])) * 0.25 for n in g[0][0]})
        plain.update()
        assert plain.grad_norm() == r0[f"gn{cycle}"] == r1[f"gn{cycle}"] and (plain.grad_norm() >= 1.0) == bool(cycle)
    for k in ("p", "m", "v"):
        assert torch.equal(getattr(plain, k).cpu(), r0[k]), k
    for r in (r0, r1):
        assert r["ngraphs"] == 4 and r["vmicro0"] == 0 and r["vcount0"] == 0
        assert r["vcalls1"] == 0 and not r["vmoved1"] and r["vcalls2"] == r["vbuckets"] > 1 and r["vmoved2"] and r["vcount"] == 1
        assert r["vloss"] == r["vloss"]
    assert torch.equal(r0["vp"], r1["vp"]) and torch.isfinite(r0["vp"]).all()
