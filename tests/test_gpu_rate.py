"""The rate term of quantisation-aware training on the GPU: vvae_latent_rate / vvae_latent_rate_grad (csrc/quant.hip) and ops.latent_rate against
quant.rate_reference, an exact family that no summation order and no missed element survives, the refusals, the op inside a captured graph,
inside the eager and the graphed train step of both VideoVAE flavours, through ``train --rate-weight``, and the descent the term is for."""
import gc
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from video_vae_amd.quant import code_counts, entropy_bits, qmax_of, quantise_reference, rate_cost_reference, rate_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 32          # infer.model_config(SMALL, True): 32 x 32 frames, hw = 4, ld = 96
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# (frames, hw, ld): one group; a few tokens; exactly the cached limit (12 groups per thread); one token past it (the re-reading form); the
# largest ld
SHAPES = [(1, 1, 8), (3, 4, 96), (5, 256, 96), (2, 257, 96), (2, 7, 1024)]
SENTINEL = -7.0


def _bits_of(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _data(frames, hw, ld, bits, seed):
    """tests/test_gpu_quant_train.py's recipe: float32 (frames, hw, ld) of bf16-representable values with channel 1 all zero; channel 2 one
    huge outlier; channel 3 amax == qmax (inv == 1) and ties k + 0.5 of both signs; channel 4 a negative maximum; channel 5 tiny values
    (amax below 1e-30: dead)."""
    qmax = qmax_of(bits)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((frames, hw, ld)) * rng.uniform(0.01, 4.0, size=(frames, 1, ld))
    x = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float().numpy()
    x[:, :, 1] = 0.0
    x[:, :, 2] *= 1e-2
    x[:, hw // 2, 2] = -3.0e4
    k = (np.arange(hw) % qmax).astype(np.float32)
    x[:, :, 3] = (k + 0.5) * np.where(np.arange(hw) % 2, -1.0, 1.0).astype(np.float32)
    x[:, 0, 3] = qmax
    x[:, :, 4] = -np.abs(x[:, :, 4]) - 0.125
    x[:, :, 5] = 1e-32
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def _keeps(frames):
    keeps = [np.ones(frames, dtype=np.float32), np.zeros(frames, dtype=np.float32)]      # all kept; every frame dropped
    mid = np.ones(frames, dtype=np.float32)
    mid[0] = 2.5                                                                         # any nonzero flag keeps
    if frames >= 2:
        mid[frames // 2] = 0.0                                                           # a dropped frame (in the middle from 3 frames on)
    return [mid] + keeps


def _gs(frames):
    """Incoming gradients, one per frame: a negative entry and, from two frames on, a zero (in the last frame, which _keeps keeps)."""
    g = np.linspace(-1.5, 2.0, frames).astype(np.float32)
    if frames > 1:
        g[-1] = 0.0
    return g


def _entries(x, keep, cost, g, bits):
    """Both C entries on sentinel-filled outputs -> (rate, grad)."""
    from video_vae_amd import ops
    from video_vae_amd._lib import check, lib
    frames, hw, ld = x.shape
    rate = torch.full((frames,), SENTINEL, device=x.device)
    grad = torch.full_like(x, SENTINEL)
    check(lib().vvae_latent_rate(ops._p(x), ops.DT[x.dtype], ops._p(keep), ops._p(cost), ops._p(rate), frames, hw, ld, bits, ops._stream()),
          "vvae_latent_rate")
    check(lib().vvae_latent_rate_grad(ops._p(x), ops.DT[x.dtype], ops._p(keep), ops._p(cost), ops._p(g), ops._p(grad), frames, hw, ld, bits,
                                      ops._stream()), "vvae_latent_rate_grad")
    return rate, grad


def _case(frames, hw, ld, dtype, bits):
    x = _data(frames, hw, ld, bits, seed=frames * 1000 + hw + bits)
    if dtype == "fp32" and ld > 6:                         # values bf16 cannot hold: the fp32 products round for real
        x[:, :, 6:] = (x[:, :, 6:] * np.float32(1.0009765625) + np.float32(3e-5)).astype(np.float32)
    cost = rate_cost_reference(code_counts(quantise_reference(x, bits)[0]), bits)
    return x, cost


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("frames,hw,ld", SHAPES)
def test_gradient_equals_the_reference_on_every_bit(dev, frames, hw, ld, dtype, bits):
    """grad = T(g slope) of quant.rate_reference, bit for bit (zero words where the frame is dropped or its g is zero), from the C entry on a
    sentinel-filled buffer and from the operator's backward pass; x is only read."""
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    assert ops.latent_quantise_supported(hw, ld, dt)
    x, cost = _case(frames, hw, ld, dtype, bits)
    g = _gs(frames)
    ct, gt = torch.from_numpy(cost).to(dev), torch.from_numpy(g).to(dev)
    for keep in _keeps(frames):
        xt = torch.from_numpy(x).to(dev).to(dt)
        before = xt.clone()
        kd = torch.from_numpy(keep).to(dev)
        _, slope = rate_reference(x, keep, bits, cost)
        want = np.where(((g == 0) | (keep == 0))[:, None, None], np.float32(0), (g[:, None, None] * slope).astype(np.float32))
        want = torch.from_numpy(want.astype(np.float32)).to(dt).to(dev)
        _, grad = _entries(xt, kd, ct, gt, bits)
        assert torch.equal(_bits_of(grad), _bits_of(want)), keep.tolist()
        assert torch.equal(_bits_of(xt), _bits_of(before))
        leaf = xt.clone().requires_grad_(True)
        kl = kd.clone().requires_grad_(True)
        rate = ops.latent_rate(leaf, kl, bits, ct)
        rate.backward(gt)
        assert leaf.grad.dtype == dt and torch.equal(_bits_of(leaf.grad), _bits_of(want)) and kl.grad is None, keep.tolist()


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("frames,hw,ld", SHAPES)
def test_rate_against_the_reference(dev, frames, hw, ld, dtype, bits):
    """rate[f] against the float64 sum of the reference's fp32 terms, within hw ld 2^-24 sum|term|: the worst case of any fp32 summation
    order over hw ld terms.  Tables from quant.rate_cost_reference; 0 for a dropped frame; twice the same bits."""
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    x, cost = _case(frames, hw, ld, dtype, bits)
    ct, gt = torch.from_numpy(cost).to(dev), torch.from_numpy(_gs(frames)).to(dev)
    for keep in _keeps(frames):
        xt = torch.from_numpy(x).to(dev).to(dt)
        kd = torch.from_numpy(keep).to(dev)
        terms, _ = rate_reference(x, keep, bits, cost)
        exact = terms.astype(np.float64).sum(axis=(1, 2))
        bound = hw * ld * 2.0 ** -24 * np.abs(terms).astype(np.float64).sum(axis=(1, 2))
        rate, _ = _entries(xt, kd, ct, gt, bits)
        got = rate.cpu().numpy().astype(np.float64)
        err = np.abs(got - exact)
        print(f"{frames}x{hw}x{ld} {dtype} b{bits} keep {keep.tolist()}: max |rate - exact| {err.max():.3e}, bound {bound.max():.3e}")
        assert np.all(err <= bound), (keep.tolist(), got, exact)
        assert np.all(got[keep == 0] == 0.0)
        op = ops.latent_rate(xt, kd, bits, ct)
        assert op.shape == (frames,) and op.dtype == torch.float32 and torch.equal(_bits_of(op), _bits_of(rate))
    x4 = torch.from_numpy(x).to(dev).to(dt).reshape(1, frames, hw, ld)             # leading dimensions pass through; keep (b, t, 1, 1)
    op4 = ops.latent_rate(x4, torch.ones(1, frames, 1, 1, device=dev), bits, ct)
    assert op4.shape == (1, frames)


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_exact_family_at_zero_tolerance(dev, dtype, bits):
    """No element may be missed or counted twice, in either form of the kernel: a table of multiples of 1/4 in [0, 2], a value qmax in every
    channel (inv == 1), x in multiples of 1/4 (1/2 for bf16 at 8 bits, which holds 126.5 but not 126.25).  Every term is then a multiple
    of 2^-4 of at most 4 and every partial sum a multiple of 2^-4 below 2^20: exact in fp32 in any order, so rate must EQUAL the sum, and
    with g a power of two grad must equal g d."""
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    qmax = qmax_of(bits)
    rng = np.random.default_rng(bits)
    cost = np.zeros(256, dtype=np.float32)
    cost[128 - qmax:129 + qmax] = rng.integers(0, 9, size=2 * qmax + 1).astype(np.float32) / 4
    den = 2 if (dtype == "bf16" and bits == 8) else 4
    for frames, hw, ld in [(2, 257, 96), (2, 256, 96), (2, 7, 1024)]:
        x = (rng.integers(-qmax * den, qmax * den + 1, size=(frames, hw, ld)) / den).astype(np.float32)
        x[:, 0, :] = qmax * np.where(np.arange(ld) % 2, -1.0, 1.0)
        xt = torch.from_numpy(x).to(dev).to(dt)
        assert np.array_equal(xt.float().cpu().numpy(), x)
        keep = np.ones(frames, dtype=np.float32)
        terms, slope = rate_reference(x, keep, bits, cost)
        assert np.array_equal(terms * 16, np.rint(terms * 16)) and float(np.abs(terms).sum()) < 2 ** 20
        want_rate = terms.astype(np.float64).sum(axis=(1, 2))
        g = np.array([0.5, -4.0], dtype=np.float32)
        rate, grad = _entries(xt, torch.from_numpy(keep).to(dev), torch.from_numpy(cost).to(dev), torch.from_numpy(g).to(dev), bits)
        assert np.array_equal(rate.cpu().numpy().astype(np.float64), want_rate), (frames, hw, ld)
        want_grad = (g[:, None, None] * slope).astype(np.float32)
        assert np.array_equal(grad.float().cpu().numpy(), want_grad), (frames, hw, ld)
        leaf = xt.clone().requires_grad_(True)
        op = ops.latent_rate(leaf, torch.ones(frames, device=dev), bits, torch.from_numpy(cost).to(dev))
        op.backward(torch.from_numpy(g).to(dev))
        assert np.array_equal(op.detach().cpu().numpy().astype(np.float64), want_rate)
        assert np.array_equal(leaf.grad.float().cpu().numpy(), want_grad)


def test_refusals_leave_the_outputs_alone(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError, check, lib
    x = torch.randn(2, 4, 96, device=dev)
    keep = torch.ones(2, device=dev)
    cost = torch.rand(256, device=dev)
    for bad in (lambda: ops.latent_rate(x, keep, 1, cost), lambda: ops.latent_rate(x, keep, 9, cost),
                lambda: ops.latent_rate(x, torch.ones(3, device=dev), 8, cost),
                lambda: ops.latent_rate(x, torch.ones(2, dtype=torch.int32, device=dev), 8, cost),
                lambda: ops.latent_rate(x.transpose(0, 1), torch.ones(4, device=dev), 8, cost),
                lambda: ops.latent_rate(x.half(), keep, 8, cost), lambda: ops.latent_rate(x, keep.cpu(), 8, cost),
                lambda: ops.latent_rate(x.cpu(), keep, 8, cost), lambda: ops.latent_rate(x, keep, 8, cost.cpu()),
                lambda: ops.latent_rate(x, keep, 8, cost[:255]), lambda: ops.latent_rate(x, keep, 8, cost.double())):
        with pytest.raises(VvaeError):
            bad()
    # the C entries: a shape they do not take, bad bits and frames, null pointers, misalignment, a gradient buffer over x
    buf = torch.randn(2 * 4 * 96 + 8, device=dev)
    src = buf[:768].view(2, 4, 96)
    kept_src = src.clone()
    rate = torch.full((2,), SENTINEL, device=dev)
    grad = torch.full((2, 4, 96), SENTINEL, device=dev)
    g = torch.ones(2, device=dev)
    fwd = lambda s, k, c, r, frames=2, hw=4, ld=96, bits=8: lib().vvae_latent_rate(
        ops._p(s), 0, ops._p(k), ops._p(c), ops._p(r), frames, hw, ld, bits, ops._stream())
    bwd = lambda s, k, c, gg, d, frames=2, hw=4, ld=96, bits=8: lib().vvae_latent_rate_grad(
        ops._p(s), 0, ops._p(k), ops._p(c), ops._p(gg), ops._p(d), frames, hw, ld, bits, ops._stream())
    codes = [fwd(src, keep, cost, rate, ld=12), fwd(src, keep, cost, rate, ld=100), fwd(src, keep, cost, rate, bits=9),
             fwd(src, keep, cost, rate, bits=1), fwd(src, keep, cost, rate, frames=0), fwd(None, keep, cost, rate),
             fwd(src, None, cost, rate), fwd(src, keep, None, rate), fwd(src, keep, cost, None), fwd(buf[1:769], keep, cost, rate),
             bwd(src, keep, cost, g, grad, ld=12), bwd(src, keep, cost, g, grad, bits=9), bwd(src, keep, cost, g, grad, frames=0),
             bwd(None, keep, cost, g, grad), bwd(src, None, cost, g, grad), bwd(src, keep, None, g, grad), bwd(src, keep, cost, None, grad),
             bwd(src, keep, cost, g, None), bwd(buf[1:769], keep, cost, g, grad), bwd(src, keep, cost, g, buf[1:769]),
             bwd(src, keep, cost, g, src), bwd(src, keep, cost, g, buf[4:772]), bwd(buf[8:776], keep, cost, g, src)]
    for code in codes:
        assert code == 1001
        with pytest.raises(VvaeError):
            check(code, "vvae_latent_rate")
    torch.cuda.synchronize()
    assert torch.equal(src, kept_src) and bool((rate == SENTINEL).all()) and bool((grad == SENTINEL).all())
    assert fwd(src, keep, cost, rate) == 0 and bwd(src, keep, cost, g, grad) == 0      # the same calls, well formed: taken
    torch.cuda.synchronize()
    assert not bool((rate == SENTINEL).any()) and not bool((grad == SENTINEL).any()) and torch.equal(src, kept_src)


def test_quantiser_bit_for_bit_with_the_parent(dev):
    """Every member of tests/golden/quant_parent_bits.json (make_quant_parent_bits.py: codes, steps, counts and the dequantised latent of
    ops.latent_quantise, the output and counts of ops.latent_fake_quant, rate[f] and the gradient of ops.latent_rate, at SHAPES, both dtypes,
    bits 2, 4, 8 and the three keep patterns), recorded on the GPU before the four kernels shared their front end, frame loop and launch path:
    same dtype, same shape, same bytes -- rate[f] included, which the bound above would let move."""
    golden = os.path.join(ROOT, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_quant_parent_bits", os.path.join(golden, "make_quant_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = mod.describe(mod.record(sys.modules[__name__], dev))
    with open(os.path.join(golden, "quant_parent_bits.json")) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want) and len(want) == len(SHAPES) * 2 * 3 * 3 * 8, (len(got), len(want), sorted(set(got) ^ set(want))[:8])
    bad = [f"{m}: got {got[m]}, recorded {want[m]}" for m in sorted(want) if got[m] != want[m]]
    assert not bad, f"{len(bad)} of {len(want)} members differ from what the parent computed; first: {bad[0]}; all: {[b.split(':')[0] for b in bad]}"


def test_captured_and_replayed_equals_eager(dev):
    """The op's forward and backward inside a captured graph, replayed with other contents in the static input, keep flags, table and
    incoming gradient: bitwise the eager results; the graph holds two kernel nodes' worth of work and no memset node."""
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    frames, hw, ld, bits = 5, 16, 96, 6
    datas = [torch.from_numpy(_data(frames, hw, ld, bits, seed=s)).to(dev).to(torch.bfloat16) for s in (1, 2)]
    keeps = [torch.tensor([1, 1, 0, 1, 1.0], device=dev), torch.tensor([0, 1, 1, 1, 0.0], device=dev)]
    costs = [torch.from_numpy(rate_cost_reference(code_counts(quantise_reference(d.float().cpu().numpy(), bits)[0]), bits)).to(dev) for d in datas]
    gs = [torch.tensor([1, -2, 3, 0, 0.5], device=dev), torch.tensor([0.25, 0, -1, 1, 2.0], device=dev)]

    def eager(i):
        leaf = datas[i].clone().requires_grad_(True)
        rate = ops.latent_rate(leaf, keeps[i], bits, costs[i])
        (grad,) = torch.autograd.grad(rate, leaf, gs[i])
        return rate.detach(), grad
    static = datas[0].clone().requires_grad_(True)
    keep, cost, g = keeps[0].clone(), costs[0].clone(), gs[0].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        torch.autograd.grad(ops.latent_rate(static, keep, bits, cost), static, g)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        rate = ops.latent_rate(static, keep, bits, cost)
        (grad,) = torch.autograd.grad(rate, static, g)
    census = graph_node_census(graph)
    assert census is not None and census.get("memset", 0) == 0 and census.get("kernel", 0) >= 2, census
    for i in (0, 1, 0):
        with torch.no_grad():
            static.copy_(datas[i])
        keep.copy_(keeps[i])
        cost.copy_(costs[i])
        g.copy_(gs[i])
        graph.replay()
        torch.cuda.synchronize()
        want_rate, want_grad = eager(i)
        assert torch.equal(_bits_of(rate.detach()), _bits_of(want_rate)) and torch.equal(_bits_of(grad), _bits_of(want_grad)), i
        assert torch.equal(static.detach(), datas[i]), i


def _small(flavour, seed=2):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    from video_vae_amd import rl_model
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _batch(dev, seed=5, b=2, t=8):
    video = torch.rand((b, t, SMALL, SMALL, 3), generator=torch.Generator().manual_seed(seed)).to(dev).to(torch.bfloat16)
    mask = torch.ones(b, t)
    mask[1, t - 2:] = 0
    return video, mask.to(dev)


def _encoder_grads(opt):
    return {name: opt.g[o:o + p.numel()].clone() for name, p, o in zip(opt.names, opt.params, opt.offsets) if name.startswith("encoder.")}


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_train_step_eager_and_graphed_with_the_rate_term(dev, flavour, monkeypatch):
    """quant_bits = 6, rate_weight = 0.01: one eager L.train_step gives finite encoder gradients that differ from those of the step without
    the key; the captured step holds no memset node and its replayed loss and rate_bpp are bitwise the eager ones on the same noise;
    rate_bpp is finite and > 0 and the loss is the quantiser-only loss plus 0.01 rate_bpp.  Without the key the loss is bitwise what it
    was before the term was ever switched on and ops.latent_rate is not entered."""
    import video_vae_amd as V
    from video_vae_amd import loss as L, ops, optim
    from video_vae_amd.graph import GraphedTrainStep
    hw = (SMALL // 16) ** 2
    base = dict(L.HPARAMS, quant_bits=6)
    hparams = dict(base, rate_weight=0.01)
    calls = []
    real = ops.latent_rate
    monkeypatch.setattr(ops, "latent_rate", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):                     # the driver's rule: ONE non-default stream for the whole run
        video, mask = _batch(dev)
        m = _small(flavour).to(dev)
        opt = optim.Optimizer(m, 0.0)                                           # lr = 0: the weights never move, so passes can be compared
        loss_q, aux_q = L.train_step(m, opt, video, mask, base, hw, V.Rngs(3))
        grads_q = _encoder_grads(opt)
        assert not calls and "rate_bpp" not in aux_q and m._quant_rate is None
        loss_q = loss_q.clone()
        loss_r, aux_r = L.train_step(m, opt, video, mask, hparams, hw, V.Rngs(3))
        grads_r = _encoder_grads(opt)
        assert len(calls) == 1 and m.latent_rate_on and torch.isfinite(loss_r)
        bpp = aux_r["rate_bpp"]
        print(f"{flavour}: loss {float(loss_q)!r} -> {float(loss_r)!r}, rate_bpp {float(bpp)!r}, code_entropy {float(aux_r['code_entropy'])!r}")
        assert torch.isfinite(bpp) and float(bpp) > 0
        assert torch.equal(loss_r, loss_q + 0.01 * bpp)                         # the same forward on the same seeds, plus the term
        differ = 0
        for name, gq in grads_q.items():
            assert bool(torch.isfinite(grads_r[name]).all()), name
            differ += int(not torch.equal(gq, grads_r[name]))
        assert differ > 0 and not torch.equal(grads_q["encoder.spatial_compression.kernel"], grads_r["encoder.spatial_compression.kernel"])
        del loss_r, aux_r, aux_q
        gc.collect()
        step = GraphedTrainStep(m, opt, video, mask, hparams, hw, V.Rngs(4), warmup=1, stream=torch.cuda.current_stream())
        assert step.census[0] is not None and all(c.get("memset", 0) == 0 for c in step.census), step.census
        video2, _ = _batch(dev, seed=6)
        for v in (video, video2):
            loss_g, aux_g = step(v, mask)
            torch.cuda.synchronize()
            loss_g, bpp_g = loss_g.clone(), aux_g["rate_bpp"].clone()
            rngs = V.Rngs(9)
            for name, (_, buf) in step.noise.items():
                rngs.inject(name, buf.clone())
            loss_e, aux_e = L.eval_step(m, v, mask, hparams, hw, rngs)           # the loss with train=True: the same forward, eagerly
            print(f"{flavour}: loss graph {float(loss_g)!r} eager {float(loss_e)!r}; rate_bpp graph {float(bpp_g)!r} eager "
                  f"{float(aux_e['rate_bpp'])!r}")
            assert torch.equal(loss_g, loss_e) and torch.equal(bpp_g, aux_e["rate_bpp"])
            assert torch.isfinite(bpp_g) and float(bpp_g) > 0
        # the switch: without the key the same model runs the quantiser-only step again, bit for bit
        n = len(calls)
        m.zero_grad(set_to_none=True)
        loss_b, aux_b = L.train_step(m, opt, video, mask, base, hw, V.Rngs(3))
        assert len(calls) == n and "rate_bpp" not in aux_b and not m.latent_rate_on and m._quant_rate is None
        assert torch.equal(loss_b, loss_q)
        for name, gq in grads_q.items():
            assert torch.equal(gq, opt.g[opt.offsets[opt.names.index(name)]:][:gq.numel()]), name
        with pytest.raises(ValueError):
            L.eval_step(m, video, mask, dict(L.HPARAMS, rate_weight=0.01), hw, V.Rngs(9))
        torch.cuda.synchronize()


def _train(args, timeout=300, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "video_vae_amd.train"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r


def test_train_driver_switches_the_rate_term_on(dev):
    """train --quantise-bits 6 --quantise-after 4 --rate-weight 0.01: rate_bpp from step 4 on and only there, two captures, no nan;
    --rate-weight without --quantise-bits is the parser's error."""
    common = ["--small", "--size", "32", "--per_device_batch_size", "2", "--max_frames", "8", "--steps", "8", "--log_every", "1"]
    out = _train(common + ["--quantise-bits", "6", "--quantise-after", "4", "--rate-weight", "0.01"]).stdout
    lines = [l for l in out.splitlines() if l.startswith("Epoch 0, Step ")]
    assert [int(l.split("Step ")[1].split(":")[0]) for l in lines] == list(range(8)), out
    for i, l in enumerate(lines):
        assert ("rate_bpp = " in l) == (i >= 4) and ("code_entropy = " in l) == (i >= 4), l
    assert "nan" not in out.lower(), out
    assert out.count("captured the train step") == 2 and "capture failed" not in out, out
    modes = [l.split("mode = ")[1].split(",")[0] for l in lines]
    assert modes == ["eager"] + ["hipgraph"] * 7, modes
    for l in lines[4:]:
        assert 0.0 < float(l.split("rate_bpp = ")[1].split(",")[0]) < 6.0 * 4 * 96 / (SMALL * SMALL) * 2, l
    r = _train(common + ["--rate-weight", "0.01"], ok=False)
    assert r.returncode == 2 and "--rate-weight needs --quantise-bits" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.parametrize("bits", [4, 6])
def test_descent_on_the_device_lowers_the_entropy_of_the_codes(dev, bits):
    """tests/test_rate_host.py's loop with the kernels: 50 plain gradient steps of 0.02 on the sum of ops.latent_rate over free
    standard-normal values (4, 64, 16), the table rebuilt every step from the quantiser kernel's counts (loss.rate_cost_table): the
    zeroth-order entropy of the codes ends at no more than 2/3 of where it started."""
    from video_vae_amd import loss as L, ops
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((4, 64, 16)).astype(np.float32)).to(dev)
    keep = torch.ones(4, device=dev)

    def counts_of(t):
        counts = torch.empty((4, 256), dtype=torch.int32, device=dev)
        ops.latent_fake_quant(t, keep, bits, counts)
        return counts
    start = entropy_bits(counts_of(x).cpu().numpy().sum(0))
    assert abs(start - entropy_bits(code_counts(quantise_reference(x.cpu().numpy(), bits)[0]))) < 1e-12
    for _ in range(50):
        cost = L.rate_cost_table(counts_of(x), bits)
        leaf = x.clone().requires_grad_(True)
        ops.latent_rate(leaf, keep, bits, cost).sum().backward()
        x = x - 0.02 * leaf.grad
    end = entropy_bits(counts_of(x).cpu().numpy().sum(0))
    print(f"bits {bits}: entropy {start:.3f} -> {end:.3f} ({end / start:.3f} of the start)")
    assert end <= start * 2 / 3
