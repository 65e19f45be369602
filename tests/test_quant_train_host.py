"""Quantisation-aware training without a GPU: quant.fake_quant_reference (the definition), ops.latent_fake_quant on CPU tensors against it on
every bit, the straight-through gradient, both VideoVAE flavours with ``latent_quant_bits``, the loss's switch and entropy, the train flags
and the ABI entry."""
import numpy as np
import pytest
import torch

from video_vae_amd.quant import dequantise_reference, entropy_bits, fake_quant_reference, qmax_of, quantise_reference

SMALL = 32          # infer.model_config(SMALL, True): 32 x 32 frames, hw = 4, ld = 96
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
SHAPES = [(1, 1, 8), (3, 5, 8), (2, 7, 1024), (5, 256, 96), (2, 3073, 8)]


def _bits_of(t):
    """The bit patterns of a bf16 / fp32 tensor: comparisons below are on integers, so NaNs and the sign of zero count."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _data(frames, hw, ld, bits, seed, fp32):
    """float32 (frames, hw, ld): channel 1 all zero, channel 2 holds an infinity, channel 3 amax == qmax (inv == step == 1) with ties
    k + 0.5 of both signs, channel 4 a negative maximum; bf16-representable unless ``fp32``."""
    qmax = qmax_of(bits)
    rng = np.random.default_rng(seed)
    x = _bf16(rng.standard_normal((frames, hw, ld)) * rng.uniform(0.01, 4.0, size=(frames, 1, ld)))
    if fp32:
        x = (x * np.float32(1.0009765625) + np.float32(3e-5)).astype(np.float32)
    x[:, :, 1] = 0.0
    x[:, hw // 2, 2] = np.inf
    k = (np.arange(hw) % qmax).astype(np.float32)
    x[:, :, 3] = (k + 0.5) * np.where(np.arange(hw) % 2, -1.0, 1.0).astype(np.float32)
    x[:, 0, 3] = qmax
    x[:, :, 4] = -np.abs(x[:, :, 4]) - 0.125
    return x


def test_reference_is_dequantise_of_quantise_on_kept_frames_and_the_input_elsewhere():
    bits = 4
    x = _data(4, 6, 16, bits, seed=1, fp32=True)
    x[2, 1, 7] = np.float32(np.nan)
    x.view(np.uint32)[2, 2, 7] = 0x7fc01234                 # a NaN with a payload, in the dropped frame
    keep = np.array([1.0, 2.5, 0.0, 1.0], dtype=np.float32)
    for dtype in ("float32", "bfloat16", torch.float32, torch.bfloat16, np.float32):
        out = fake_quant_reference(x, keep, bits, dtype)
        assert out.dtype == np.float32 and out.shape == x.shape
        want = dequantise_reference(*quantise_reference(x, bits))
        if "bfloat16" in str(dtype):
            want = _bf16(want)
        k = keep != 0
        assert np.array_equal(out[k].view(np.uint32), want[k].view(np.uint32))
        assert np.array_equal(out[~k].view(np.uint32), x[~k].view(np.uint32))        # bit for bit, NaN payloads included
    assert np.array_equal(fake_quant_reference(x, np.zeros(4), bits, "float32").view(np.uint32), x.view(np.uint32))
    with pytest.raises(ValueError):
        fake_quant_reference(x, keep, 9, "float32")
    with pytest.raises(ValueError):
        fake_quant_reference(x, np.zeros(4), 1, "float32")
    with pytest.raises(ValueError):
        fake_quant_reference(x, keep[:3], bits, "float32")
    with pytest.raises(ValueError):
        fake_quant_reference(x, keep, bits, "float16")


def test_reference_code_zero_is_plus_zero():
    """The value goes through the integer code: whatever rounds to code 0 comes back as +0.0, also from a negative input, where
    rint(x * inv) * step keeps the sign."""
    x = np.array([[[-0.01], [0.01], [-0.0], [-1.0]]], dtype=np.float32).repeat(8, axis=2)
    out = fake_quant_reference(x, np.ones(1), 4, "float32")
    assert np.array_equal(out[0, :3].view(np.uint32), np.zeros((3, 8), dtype=np.uint32))
    assert np.all(out[0, 3] == -1.0)
    naive = np.rint(x * np.float32(7.0)) * np.float32(1.0 / 7.0)
    assert np.signbit(naive[0, 0]).all() and not np.signbit(out[0, 0]).any()
    for dt in DTYPES.values():
        from video_vae_amd import ops
        got = ops.latent_fake_quant(torch.from_numpy(x).to(dt), torch.ones(1), 4)
        assert torch.equal(_bits_of(got[0, :3]), torch.zeros_like(_bits_of(got[0, :3])))


@pytest.mark.parametrize("bits", [2, 4, 6, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("frames,hw,ld", SHAPES)
def test_cpu_operator_equals_the_reference_on_every_bit(frames, hw, ld, dtype, bits):
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    x = _data(frames, hw, ld, bits, seed=frames * 1000 + hw + bits, fp32=dtype == "fp32")
    keeps = [np.ones(frames, dtype=np.float32), np.zeros(frames, dtype=np.float32)]
    if frames >= 2:
        mid = np.ones(frames, dtype=np.float32)
        mid[frames // 2] = 0.0
        mid[0] = 2.5
        keeps.insert(0, mid)
        x[frames // 2, 0, 5:8] = np.float32(np.nan)             # a NaN inside the frame that keeps[0] drops
    for keep in keeps:
        xt = torch.from_numpy(x).to(dt)
        before = xt.clone()
        counts = torch.full((frames, 256), -7, dtype=torch.int32)
        got = ops.latent_fake_quant(xt, torch.from_numpy(keep), bits, counts)
        want = torch.from_numpy(fake_quant_reference(xt.float().numpy(), keep, bits, dt)).to(dt)
        assert got.dtype == dt and got.shape == xt.shape and got.data_ptr() != xt.data_ptr()
        assert torch.equal(_bits_of(got), _bits_of(want)), keep.tolist()
        assert torch.equal(_bits_of(xt), _bits_of(before))
        q, _ = quantise_reference(xt.float().numpy(), bits)
        ref_counts = np.stack([np.bincount(q[f].astype(np.int64).reshape(-1) + 128, minlength=256) if keep[f] != 0 else np.zeros(256, dtype=np.int64)
                               for f in range(frames)])
        assert np.array_equal(counts.numpy().astype(np.int64), ref_counts), keep.tolist()
        assert torch.equal(_bits_of(ops.latent_fake_quant(xt, torch.from_numpy(keep), bits)), _bits_of(want))     # counts=None
    # leading dimensions pass through; keep may carry trailing unit dimensions, as the models' selections do
    x4 = torch.from_numpy(x).to(dt).reshape(1, frames, hw, ld)
    got = ops.latent_fake_quant(x4, torch.ones(1, frames, 1, 1), bits)
    assert got.shape == x4.shape


@pytest.mark.parametrize("bits", [2, 4, 6, 8])
def test_ties_round_to_even_in_bf16(bits):
    """amax == qmax makes inv == step == 1: k + 0.5 is representable in bf16 up to 8 bits (126.5 needs 8 significant bits) and rounds
    to the even neighbour."""
    from video_vae_amd import ops
    qmax = qmax_of(bits)
    k = np.arange(qmax, dtype=np.float32)
    col = np.concatenate([k + 0.5, -(k + 0.5), [np.float32(qmax)]]).astype(np.float32)
    assert np.array_equal(_bf16(col), col)
    x = np.zeros((1, col.size, 8), dtype=np.float32)
    x[0, :, 0] = col
    even = np.concatenate([np.rint(k + 0.5), -np.rint(k + 0.5), [qmax]]).astype(np.float32)
    assert np.all(even[:-1] % 2 == 0)
    for dt in DTYPES.values():
        got = ops.latent_fake_quant(torch.from_numpy(x).to(dt), torch.ones(1), bits)
        assert np.array_equal(got.float().numpy()[0, :, 0], even)
        assert np.array_equal(fake_quant_reference(x, np.ones(1), bits, dt)[0, :, 0], even)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_gradient_is_the_incoming_gradient(dtype):
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 5, 16), generator=g).to(dt).requires_grad_(True)
    keep = torch.tensor([1.0, 0.0, 1.0], requires_grad=True)
    y = ops.latent_fake_quant(x, keep, 4)
    assert y.requires_grad
    gy = torch.randn((3, 5, 16), generator=g).to(dt)
    y.backward(gy)
    assert torch.equal(_bits_of(x.grad), _bits_of(gy)) and keep.grad is None


def test_refusals_before_any_work():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    x, keep = torch.zeros(2, 4, 8), torch.ones(2)
    for bad in (lambda: ops.latent_fake_quant(x, keep, 1), lambda: ops.latent_fake_quant(x, keep, 9),
                lambda: ops.latent_fake_quant(x, torch.ones(3), 4), lambda: ops.latent_fake_quant(x, torch.ones(2, dtype=torch.int32), 4),
                lambda: ops.latent_fake_quant(x.transpose(0, 1), torch.ones(4), 4), lambda: ops.latent_fake_quant(x.half(), keep, 4),
                lambda: ops.latent_fake_quant(x, keep, 4, torch.zeros(2, 256)), lambda: ops.latent_fake_quant(x, keep, 4, torch.zeros(3, 256, dtype=torch.int32)),
                lambda: ops.latent_fake_quant(x, keep.to("meta"), 4)):
        with pytest.raises(VvaeError):
            bad()


def _small(flavour, seed=2):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    from video_vae_amd import rl_model
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _cpu_trunk(monkeypatch):
    """The attention trunks, the reparameterisation kernel and the UNet run on a GPU only (ops: no CPU path), so a CPU forward reaches
    VideoVAE.forward's own code -- heads, gate, quantiser, the order of the noise draws -- with stand-ins for those three: patch pixels as
    the encoder's features, the decoder's first Linear as the decoder, z = mean + eps exp(logvar / 2) from framework ops.  The whole
    model runs in tests/test_gpu_quant_train.py."""
    from einops import rearrange
    from video_vae_amd import model as M, ops
    monkeypatch.setattr(M.Encoder, "_features",
                        lambda self, x, mask: rearrange(x - 0.5, "b t (h p) (w q) c -> b t (h w) (p q c)", p=16, q=16).to(self.dtype))
    monkeypatch.setattr(M.Decoder, "forward", lambda self, x, mask, rngs, train=True: self.spatial_decompression(x))
    monkeypatch.setattr(ops, "reparameterise_kl", lambda mean, logvar, eps, mask_bt:
                        (mean.float() + eps.float() * torch.exp(0.5 * logvar.float()), torch.zeros(mean.shape[0])))


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_model_forward_quantises_the_gated_latent(flavour, train, monkeypatch):
    """CPU forward with latent_quant_bits = 4 against the plain forward on equal seeds: the compressed representation it returns (and
    decodes) is the reference applied to the plain run's, with the plain run's hard selection; with None the op is never entered."""
    import video_vae_amd as V
    from video_vae_amd import ops
    _cpu_trunk(monkeypatch)
    m = _small(flavour)
    assert m.latent_quant_bits is None
    b, t, bits = 2, 4, 4
    video = torch.rand((b, t, SMALL, SMALL, 3), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(b, 1, 1, t)
    calls = []
    real = ops.latent_fake_quant
    monkeypatch.setattr(ops, "latent_fake_quant", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        m.encoder.selection_layer2.bias.fill_(-1.0)                                 # logits around 0: kept and dropped frames both occur
        plain = m(video, mask, V.Rngs(7), train=train)
        assert not calls and m._quant_counts is None
        m.latent_quant_bits = bits
        quant = m(video, mask, V.Rngs(7), train=train)
    assert len(calls) == 1
    comp_p, comp_q = plain[1], quant[1]
    keep = (plain[3] if flavour == "rl" else plain[2]).reshape(-1).float().numpy()
    assert comp_p.shape[-2:] == (4, 96) and keep.size == comp_p.numel() // (4 * 96)
    for a, c in zip(plain[2:], quant[2:]):                                          # selection, log-variance and mean do not move
        assert torch.equal(a, c)
    frames = keep.size
    want = fake_quant_reference(comp_p.float().reshape(frames, 4, 96).numpy(), keep, bits, comp_p.dtype)
    assert comp_q.dtype == comp_p.dtype
    assert torch.equal(_bits_of(comp_q.reshape(frames, 4, 96)), _bits_of(torch.from_numpy(want).to(comp_p.dtype)))
    if train:
        assert 0 < np.count_nonzero(keep) < frames                                  # the seed gives both kinds of frame
    if keep.any():
        assert not torch.equal(comp_q, comp_p) and not torch.equal(quant[0], plain[0])
    counts = m._quant_counts
    assert counts.shape == tuple(comp_q.shape[:-2]) + (256,) and int(counts.sum()) == np.count_nonzero(keep) * 4 * 96


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_gradients_pass_the_quantiser_unchanged(flavour, monkeypatch):
    """Straight-through inside the model: with the stand-in decoder (linear in its input), the gradient at the gated latent is the same
    tensor with the quantiser on and off, so the heads' and the gate's gradients arrive unchanged."""
    import video_vae_amd as V
    _cpu_trunk(monkeypatch)
    m = _small(flavour)
    video = torch.rand((2, 4, SMALL, SMALL, 3), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(2, 1, 1, 4)
    grads = []
    for bits in (None, 4):
        m.latent_quant_bits = bits
        m.zero_grad()
        out = m(video, mask, V.Rngs(7), train=True)
        out[0].float().sum().backward()
        grads.append({k: p.grad.clone() for k, p in m.encoder.named_parameters() if p.grad is not None} | {"fill": m.fill_token.grad.clone()})
    assert grads[0].keys() == grads[1].keys() and "spatial_compression.kernel" in grads[0]
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_loss_switch_and_code_entropy():
    """loss.set_quantiser follows hparams["quant_bits"]; loss.with_rate adds code_entropy only when a forward left a histogram; the entropy
    is quant.entropy_bits of the pooled counts (0 log 0 = 0).  The losses themselves run on a GPU (tests/test_gpu_quant_train.py)."""
    from types import SimpleNamespace
    from video_vae_amd import loss as L
    m = SimpleNamespace()
    L.set_quantiser(m, dict(L.HPARAMS))
    assert not hasattr(m, "latent_quant_bits")                                      # off: a model is not touched
    L.set_quantiser(m, dict(L.HPARAMS, quant_bits=6))
    assert m.latent_quant_bits == 6
    L.set_quantiser(m, dict(L.HPARAMS))
    assert m.latent_quant_bits is None
    assert L.with_rate(m, {"MSE": 1}) == {"MSE": 1}
    rng = np.random.default_rng(0)
    c = rng.integers(0, 3000, size=(5, 256)).astype(np.int32) * (rng.random((5, 256)) < 0.3)
    c[3] = 0                                                                        # a dropped frame
    m._quant_counts = torch.from_numpy(c.astype(np.int32))
    aux = L.with_rate(m, {"MSE": 1})
    assert list(aux) == ["MSE", "code_entropy"] and abs(float(aux["code_entropy"]) - entropy_bits(c.sum(0))) <= 1e-4
    assert float(L.code_entropy(torch.zeros(3, 256, dtype=torch.int32))) == 0.0     # every frame dropped
    one = torch.zeros(2, 256, dtype=torch.int32)
    one[:, 128] = 50
    assert float(L.code_entropy(one)) == 0.0
    two = one.clone()
    two[0, 129] = 100
    assert abs(float(L.code_entropy(two)) - 1.0) <= 1e-6


def test_train_flags():
    from video_vae_amd import train
    a = train.parse_args([])
    assert a.quantise_bits is None and a.quantise_after == 0
    for n in range(2, 9):
        assert train.parse_args(["--quantise-bits", str(n)]).quantise_bits == n
    a = train.parse_args(["--quantise-bits", "6", "--quantise-after", "4"])
    assert (a.quantise_bits, a.quantise_after) == (6, 4)
    for bad in (["--quantise-bits", "1"], ["--quantise-bits", "9"], ["--quantise-after", "4"], ["--quantise-bits", "6", "--quantise-after", "-1"]):
        with pytest.raises(SystemExit):
            train.parse_args(bad)


def test_header_declares_and_library_exports_the_entry():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    assert "vvae_latent_fake_quant" in protos and len(protos["vvae_latent_fake_quant"][1]) == 10
    assert len(protos["vvae_latent_quantise"][1]) == 12                             # the existing entry keeps its signature
    assert getattr(lib(), "vvae_latent_fake_quant") is not None
