"""Quantisation-aware training on the GPU: ops.latent_fake_quant (csrc/quant.hip, vvae_latent_fake_quant) against quant.fake_quant_reference
and against clone + ops.latent_quantise(dequantise_in_place=True) on every bit, its refusals, its gradient, inside a captured graph, inside
both VideoVAE flavours, inside the eager and the graphed train step, and through ``train --quantise-bits``."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from video_vae_amd.quant import entropy_bits, fake_quant_reference, qmax_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 32          # infer.model_config(SMALL, True): 32 x 32 frames, hw = 4, ld = 96
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# (frames, hw, ld): one group; a few tokens; exactly the cached limit (12 groups per thread); one token past it (the re-reading form); the
# largest ld
SHAPES = [(1, 1, 8), (3, 4, 96), (5, 256, 96), (2, 257, 96), (2, 7, 1024)]


def _bits_of(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _data(frames, hw, ld, bits, seed):
    """tests/test_gpu_quant.py's recipe: float32 (frames, hw, ld) of bf16-representable values with channel 1 all zero; channel 2 one huge
    outlier; channel 3 amax == qmax (inv == 1) and ties k + 0.5 of both signs; channel 4 a negative maximum; channel 5 tiny values (amax
    below 1e-30: dead)."""
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


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("frames,hw,ld", SHAPES)
def test_kernel_equals_the_reference_and_the_existing_pair_on_every_bit(dev, frames, hw, ld, dtype, bits):
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    assert ops.latent_quantise_supported(hw, ld, dt)
    x = _data(frames, hw, ld, bits, seed=frames * 1000 + hw + bits)
    if dtype == "fp32" and ld > 6:                         # values bf16 cannot hold: the fp32 products round for real
        x[:, :, 6:] = (x[:, :, 6:] * np.float32(1.0009765625) + np.float32(3e-5)).astype(np.float32)
    nan_bits = {torch.bfloat16: [0x7fc1, 0x7f81, -0x3f], torch.float32: [0x7fc01234, 0x7f812345, -0x3fedcb]}[dt]
    for keep in _keeps(frames):
        src = torch.from_numpy(x).to(dev).to(dt)
        dropped = torch.from_numpy(keep == 0).to(dev)
        if bool(dropped.any()):                            # NaNs of three payloads (quiet, signalling, negative) inside a dropped frame
            f = int(dropped.nonzero()[0])
            _bits_of(src)[f].view(-1)[:3] = torch.tensor(nan_bits, dtype=_bits_of(src).dtype, device=dev)
            assert bool(torch.isnan(src[f].view(-1)[:3]).all())
        before = src.clone()
        kd = torch.from_numpy(keep).to(dev)
        counts = torch.full((frames, 256), -7, dtype=torch.int32, device=dev)
        got = ops.latent_fake_quant(src, kd, bits, counts)
        assert got.dtype == dt and got.shape == src.shape and got.data_ptr() != src.data_ptr()
        assert torch.equal(_bits_of(src), _bits_of(before)), keep.tolist()                # src is only read
        kept = ~dropped
        want = torch.from_numpy(fake_quant_reference(before.float().cpu().numpy(), keep, bits, dt)).to(dt).to(dev)
        assert torch.equal(_bits_of(got[kept]), _bits_of(want[kept])), keep.tolist()
        assert torch.equal(_bits_of(got[dropped]), _bits_of(before[dropped])), keep.tolist()      # copied through with its bits, NaN payloads too
        pair = before.clone()
        q = ops.latent_quantise(pair, kd, bits, dequantise_in_place=True)
        assert torch.equal(_bits_of(got), _bits_of(pair)), keep.tolist()
        assert torch.equal(counts, q.counts), keep.tolist()
        assert counts.sum(dim=-1).tolist() == [hw * ld if k else 0 for k in keep]
        none = ops.latent_fake_quant(src, kd, bits)                                        # counts=None
        assert torch.equal(_bits_of(none), _bits_of(got))
    # leading dimensions pass through; keep as the models hand it over, (b, t, 1, 1)
    src = torch.from_numpy(x).to(dev).to(dt).reshape(1, frames, hw, ld)
    counts = torch.empty((1, frames, 256), dtype=torch.int32, device=dev)
    got = ops.latent_fake_quant(src, torch.ones(1, frames, 1, 1, device=dev), bits, counts)
    assert got.shape == src.shape and counts.sum(dim=-1).tolist() == [[hw * ld] * frames]


def test_refusals_leave_the_outputs_alone(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError, check, lib
    x = torch.randn(2, 4, 96, device=dev)
    keep = torch.ones(2, device=dev)
    counts = torch.full((2, 256), -7, dtype=torch.int32, device=dev)
    for bad in (lambda: ops.latent_fake_quant(x, keep, 1, counts), lambda: ops.latent_fake_quant(x, keep, 9, counts),
                lambda: ops.latent_fake_quant(x, torch.ones(3, device=dev), 8, counts),
                lambda: ops.latent_fake_quant(x, torch.ones(2, dtype=torch.int32, device=dev), 8, counts),
                lambda: ops.latent_fake_quant(x.transpose(0, 1), torch.ones(4, device=dev), 8),
                lambda: ops.latent_fake_quant(x.half(), keep, 8, counts),
                lambda: ops.latent_fake_quant(x, keep.cpu(), 8, counts), lambda: ops.latent_fake_quant(x.cpu(), keep, 8),
                lambda: ops.latent_fake_quant(x, keep, 8, counts.cpu()), lambda: ops.latent_fake_quant(x, keep, 8, counts.float()),
                lambda: ops.latent_fake_quant(x, keep, 8, counts[:1])):
        with pytest.raises(VvaeError):
            bad()
    # the C entry: aliased and overlapping buffers, a shape it does not take, bad bits, null pointers
    buf = torch.randn(2 * 4 * 96 + 8, device=dev)
    dst = torch.full((2, 4, 96), 7.0, device=dev)
    entry = lambda s, d, k, c, frames=2, hw=4, ld=96, bits=8: lib().vvae_latent_fake_quant(
        ops._p(s), ops._p(d), 0, ops._p(k), ops._p(c), frames, hw, ld, bits, ops._stream())
    src = buf[:768].view(2, 4, 96)
    kept_src = src.clone()
    for code in (entry(src, src, keep, counts), entry(src, buf[4:772], keep, counts), entry(buf[8:776], src, keep, counts),
                 entry(src, dst, keep, counts, ld=12), entry(src, dst, keep, counts, ld=100), entry(src, dst, keep, counts, bits=9),
                 entry(src, dst, keep, counts, frames=0), entry(None, dst, keep, counts), entry(src, None, keep, counts),
                 entry(src, dst, None, counts), entry(src, buf[1:769], keep, counts)):
        assert code == 1001
        with pytest.raises(VvaeError):
            check(code, "vvae_latent_fake_quant")
    torch.cuda.synchronize()
    assert torch.equal(src, kept_src) and bool((dst == 7.0).all()) and bool((counts == -7).all())
    assert entry(src, dst, keep, counts) == 0                                              # the same call, disjoint: taken
    torch.cuda.synchronize()
    assert bool((counts.sum(-1) == 4 * 96).all()) and not bool((dst == 7.0).any())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_gradient_is_the_identity(dev, dtype):
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 5, 16), generator=g).to(dev).to(dt).requires_grad_(True)
    keep = torch.tensor([1.0, 0.0, 1.0], device=dev, requires_grad=True)
    y = ops.latent_fake_quant(x, keep, 4)
    gy = torch.randn((3, 5, 16), generator=g).to(dev).to(dt)
    y.backward(gy)
    assert torch.equal(_bits_of(x.grad), _bits_of(gy)) and keep.grad is None


def test_captured_and_replayed_equals_eager(dev):
    """The op inside a captured graph, replayed with other contents in the static input and keep flags: bitwise the eager results; the graph
    holds no memset node."""
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    frames, hw, ld, bits = 5, 16, 96, 6
    datas = [torch.from_numpy(_data(frames, hw, ld, bits, seed=s)).to(dev).to(torch.bfloat16) for s in (1, 2)]
    keeps = [torch.tensor([1, 1, 0, 1, 1.0], device=dev), torch.tensor([0, 1, 1, 1, 0.0], device=dev)]
    static, keep = datas[0].clone(), keeps[0].clone()
    counts = torch.empty((frames, 256), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.latent_fake_quant(static, keep, bits, counts)
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        out = ops.latent_fake_quant(static, keep, bits, counts)
    census = graph_node_census(g)
    assert census is not None and census.get("memset", 0) == 0 and census.get("kernel", 0) >= 1, census
    for i in (0, 1, 0):
        static.copy_(datas[i])
        keep.copy_(keeps[i])
        g.replay()
        want_counts = torch.empty_like(counts)
        want = ops.latent_fake_quant(datas[i], keeps[i], bits, want_counts)
        assert torch.equal(_bits_of(out), _bits_of(want)) and torch.equal(counts, want_counts), i
        assert torch.equal(static, datas[i]), i


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


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_model_decodes_the_quantised_latent(dev, flavour):
    """latent_quant_bits = 6 on the fused-heads branch and, in eval mode, on the framework branch: the tensor forward returns and decodes is
    the reference applied to the plain run's, with the plain run's hard selection, on equal seeds."""
    import video_vae_amd as V
    from video_vae_amd import loss as L
    bits = 6
    m = _small(flavour).to(dev)
    video, mask = _batch(dev)
    with torch.no_grad():
        m.encoder.selection_layer2.bias.fill_(-1.0)                                 # logits around 0: kept and dropped frames both occur
    for train in (True, False):
        with torch.no_grad():
            m.latent_quant_bits = None
            plain = m(video, L.compact_mask(mask), V.Rngs(7), train=train)
            assert m._quant_counts is None
            m.latent_quant_bits = bits
            quant = m(video, L.compact_mask(mask), V.Rngs(7), train=train)
        comp_p, comp_q = plain[1], quant[1]
        keep = (plain[3] if flavour == "rl" else plain[2]).reshape(-1).float().cpu().numpy()
        frames = keep.size
        assert comp_p.shape[-2:] == (4, 96) and frames == comp_p.numel() // (4 * 96)
        if train:
            assert comp_p.dtype == torch.bfloat16 and np.count_nonzero(keep) > 0
        for a, c in zip(plain[2:], quant[2:]):
            assert torch.equal(a, c)
        want = fake_quant_reference(comp_p.float().reshape(frames, 4, 96).cpu().numpy(), keep, bits, comp_p.dtype)
        assert comp_q.dtype == comp_p.dtype
        assert torch.equal(_bits_of(comp_q.reshape(frames, 4, 96).cpu()), _bits_of(torch.from_numpy(want).to(comp_p.dtype))), train
        if keep.any():
            assert not torch.equal(comp_q, comp_p) and not torch.equal(quant[0], plain[0])
        assert int(m._quant_counts.sum()) == np.count_nonzero(keep) * 4 * 96


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_train_step_eager_and_graphed_with_the_quantiser(dev, flavour):
    """One eager L.train_step with quant_bits = 6 leaves finite gradients on every encoder parameter (the straight-through estimator lets
    them pass); the captured step holds no memset node, its replayed loss is bitwise the eager loss on the same noise, and code_entropy is
    quant.entropy_bits of the pooled counts within 1e-4 bits (256 fp32 terms of magnitude <= 0.53 at a few ulp each: about 3e-5)."""
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim
    from video_vae_amd.graph import GraphedTrainStep
    hw = (SMALL // 16) ** 2
    hparams = dict(L.HPARAMS, quant_bits=6)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):                     # the driver's rule: ONE non-default stream for the whole run
        video, mask = _batch(dev)
        m = _small(flavour).to(dev)
        opt = optim.Optimizer(m, 0.0)                                           # lr = 0: the weights never move, so passes can be compared
        loss, aux = L.train_step(m, opt, video, mask, hparams, hw, V.Rngs(3))
        assert m.latent_quant_bits == 6 and torch.isfinite(loss) and "code_entropy" in aux
        for name, p, o in zip(opt.names, opt.params, opt.offsets):
            if name.startswith("encoder."):
                g = opt.g[o:o + p.numel()]
                assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        del loss, aux
        gc.collect()
        step = GraphedTrainStep(m, opt, video, mask, hparams, hw, V.Rngs(4), warmup=1, stream=torch.cuda.current_stream())
        assert step.census[0] is not None and all(c.get("memset", 0) == 0 for c in step.census), step.census
        video2, _ = _batch(dev, seed=6)
        for v in (video, video2):
            loss_g, aux_g = step(v, mask)
            torch.cuda.synchronize()
            loss_g, ent_g = loss_g.clone(), aux_g["code_entropy"].clone()
            rngs = V.Rngs(9)
            for name, (_, buf) in step.noise.items():
                rngs.inject(name, buf.clone())
            loss_e, aux_e = L.eval_step(m, v, mask, hparams, hw, rngs)           # the loss with train=True: the same forward, eagerly
            pooled = m._quant_counts.reshape(-1, 256).sum(0).cpu().numpy()
            want = entropy_bits(pooled)
            print(f"{flavour}: loss graph {float(loss_g)!r} eager {float(loss_e)!r}; code_entropy graph {float(ent_g)!r} eager "
                  f"{float(aux_e['code_entropy'])!r} float64 {want!r}; codes {int(pooled.sum())}")
            assert torch.equal(loss_g, loss_e)
            assert torch.equal(ent_g, aux_e["code_entropy"])
            assert 0 < int(pooled.sum()) and 0.0 < want <= 6.0
            assert abs(float(ent_g) - want) <= 1e-4
        # the switch: without the key the same model runs the plain step again
        loss_p, aux_p = L.eval_step(m, video, mask, dict(L.HPARAMS), hw, V.Rngs(9))
        assert "code_entropy" not in aux_p and m.latent_quant_bits is None and m._quant_counts is None
        torch.cuda.synchronize()


def _train(args, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "video_vae_amd.train"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_train_driver_switches_the_quantiser_on(dev):
    """train --quantise-bits 6 --quantise-after 4: code_entropy from step 4 on and only there, the shape's graph captured twice (the switch
    re-captures it), replayed steps after each capture; without the flags one capture and no code_entropy."""
    common = ["--small", "--size", "32", "--per_device_batch_size", "2", "--max_frames", "8", "--steps", "8", "--log_every", "1"]
    out = _train(common + ["--quantise-bits", "6", "--quantise-after", "4"])
    lines = [l for l in out.splitlines() if l.startswith("Epoch 0, Step ")]
    assert [int(l.split("Step ")[1].split(":")[0]) for l in lines] == list(range(8)), out
    for i, l in enumerate(lines):
        assert ("code_entropy = " in l) == (i >= 4), l
    assert "nan" not in out.lower(), out
    assert out.count("captured the train step") == 2 and "capture failed" not in out, out
    modes = [l.split("mode = ")[1].split(",")[0] for l in lines]
    assert modes == ["eager"] + ["hipgraph"] * 7, modes
    for l in lines[4:]:
        assert 0.0 < float(l.split("code_entropy = ")[1].split(",")[0]) <= 6.0, l
    plain = _train(common)
    assert "code_entropy" not in plain and plain.count("captured the train step") == 1 and "nan" not in plain.lower(), plain
