"""The rate term of quantisation-aware training without a GPU: quant.rate_cost_reference / quant.rate_reference (the definition),
ops.latent_rate on CPU tensors against them on every bit, loss.rate_cost_table, the loss's switch and sum, the descent the term is for, the
train flags and the ABI entries."""
import numpy as np
import pytest
import torch

from video_vae_amd.quant import (code_counts, entropy_bits, qmax_of, quantise_reference, rate_cost_reference, rate_reference)

SMALL = 32          # infer.model_config(SMALL, True): 32 x 32 frames, hw = 4, ld = 96
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
SHAPES = [(1, 1, 8), (3, 4, 96), (5, 256, 96), (2, 257, 96), (2, 7, 1024)]


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
    keeps = [np.ones(frames, dtype=np.float32), np.zeros(frames, dtype=np.float32)]
    mid = np.ones(frames, dtype=np.float32)
    mid[0] = 2.5
    if frames >= 2:
        mid[frames // 2] = 0.0
    return [mid] + keeps


def _table(x, bits):
    """The cost table of the codes of ``x`` itself."""
    return rate_cost_reference(code_counts(quantise_reference(x, bits)[0]), bits)


def _quarters(bits, seed=0):
    """A table of multiples of 1/4 in [0, 2] on the alphabet, 0 elsewhere: sums and differences of its entries are exact in fp32."""
    qmax = qmax_of(bits)
    c = np.zeros(256, dtype=np.float32)
    c[128 - qmax:129 + qmax] = np.random.default_rng(seed).integers(0, 9, size=2 * qmax + 1).astype(np.float32) / 4
    return c


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_cost_reference_is_the_smoothed_code_length(bits):
    qmax = qmax_of(bits)
    rng = np.random.default_rng(bits)
    counts = rng.integers(0, 5000, size=(3, 256)) * (np.abs(np.arange(256) - 128) <= qmax)
    counts[:, 128 + qmax] = 0                                   # a symbol that never occurred still has a finite price
    c = rate_cost_reference(counts, bits)
    assert c.dtype == np.float32 and c.shape == (256,)
    live = np.abs(np.arange(256) - 128) <= qmax
    assert np.all(c[~live] == 0) and np.all(c[live] > 0) and np.all(np.isfinite(c))
    n = counts.sum(0).astype(np.float64)
    want = np.log2(n.sum() + (2 * qmax + 1) * 0.5) - np.log2(n + 0.5)
    assert np.abs(c[live] - want[live]).max() <= 1.5e-5
    assert abs(np.exp2(-c[live].astype(np.float64)).sum() - 1.0) <= 1e-4          # the prices of a distribution over the alphabet
    assert np.array_equal(c, rate_cost_reference(counts.sum(0), bits))             # pooled first
    empty = rate_cost_reference(np.zeros((2, 256), dtype=np.int32), bits)
    assert np.all(empty[live] == empty[128]) and abs(float(empty[128]) - np.log2(2 * qmax + 1)) <= 1e-5 and np.all(empty[~live] == 0)
    with pytest.raises(ValueError):
        rate_cost_reference(counts, 9)


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_reference_at_integer_codes_is_the_table(bits):
    """Every v an integer (a value qmax in every channel makes inv == 1): each term is C[q + 128] -- exactly for a table whose differences
    are exact, to one rounding of the top code's ``lo + (hi - lo)`` for any table -- so the frame's rate is the table summed over its codes."""
    qmax = qmax_of(bits)
    rng = np.random.default_rng(bits)
    x = rng.integers(-qmax, qmax + 1, size=(2, 9, 16)).astype(np.float32)
    x[:, 0, :] = qmax
    x[:, 1, :] = -qmax
    q, step = quantise_reference(x, bits)
    assert np.all(step == 1) and np.array_equal(q.astype(np.float32), x)
    keep = np.ones(2, dtype=np.float32)
    exact = _quarters(bits)
    terms, slope = rate_reference(x, keep, bits, exact)
    assert terms.dtype == np.float32 and slope.dtype == np.float32 and terms.shape == x.shape == slope.shape
    assert np.array_equal(terms, exact[q.astype(np.int64) + 128])
    assert float(terms.astype(np.float64).sum()) == float(exact[q.astype(np.int64) + 128].astype(np.float64).sum())
    k = np.minimum(q.astype(np.int64), qmax - 1)
    assert np.array_equal(slope, exact[k + 129] - exact[k + 128])                  # inv == 1: the slope is the table's difference
    real = _table(x, bits)
    terms, _ = rate_reference(x, keep, bits, real)
    want = real[q.astype(np.int64) + 128]
    assert np.array_equal(terms[q < qmax], want[q < qmax])
    assert np.abs(terms - want).max() <= 2.0 ** -22 * float(np.abs(real).max())


def test_reference_dead_channels_and_dropped_frames_give_zeros():
    bits = 4
    x = _data(4, 6, 16, bits, seed=1)
    x[:, 2, 6] = np.inf                                         # not finite: dead
    x[:, 3, 7] = np.nan
    keep = np.array([1.0, 2.5, 0.0, 1.0], dtype=np.float32)
    terms, slope = rate_reference(x, keep, bits, _table(np.nan_to_num(x, posinf=0.0), bits))
    assert np.all(np.isfinite(terms)) and np.all(np.isfinite(slope))
    for c in (1, 5, 6, 7):                                      # all zero; below 1e-30; an infinity; a NaN
        assert np.all(terms[:, :, c].view(np.uint32) == 0) and np.all(slope[:, :, c].view(np.uint32) == 0), c
    assert np.all(terms[2].view(np.uint32) == 0) and np.all(slope[2].view(np.uint32) == 0)
    assert np.all(terms[[0, 1, 3]][:, :, [0, 2, 3, 4]] > 0)     # live channels of kept frames pay
    zt, zs = rate_reference(x, np.zeros(4), bits, np.ones(256, dtype=np.float32))
    assert not zt.any() and not zs.any()
    with pytest.raises(ValueError):
        rate_reference(x, keep[:3], bits, np.zeros(256, dtype=np.float32))
    with pytest.raises(ValueError):
        rate_reference(x, keep, bits, np.zeros(255, dtype=np.float32))
    with pytest.raises(ValueError):
        rate_reference(x, keep, 1, np.zeros(256, dtype=np.float32))


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_reference_fraction_is_exact(bits):
    """t = v - floor(v) has no rounding error wherever v >= 0 or v <= -1 (k = 0 keeps v's own bits; otherwise k and v lie within a factor
    of two of each other and the difference of such numbers is exact), checked against float64.  In the one cell -1 < v < 0 the sum
    1 + v can need a bit below 2^-24 (v = -2^-30 is one such value) and is rounded once, to within 2^-25: no formula in fp32 gives it
    exactly.  The term is C[k + 128] + fl(t d) built from that t."""
    qmax = qmax_of(bits)
    x = _data(3, 50, 16, bits, seed=7)
    x[:, :, 6:] = (x[:, :, 6:] * np.float32(1.0009765625) + np.float32(3e-5)).astype(np.float32)
    cost = _table(x, bits)
    keep = np.ones(3, dtype=np.float32)
    terms, slope = rate_reference(x, keep, bits, cost)
    amax = np.abs(x).max(axis=1)
    live = amax >= 1e-30
    inv = np.where(live, np.float32(qmax) / np.where(live, amax, np.float32(1)), np.float32(0)).astype(np.float32)
    v = (x * inv[:, None, :]).astype(np.float32)
    k = np.clip(np.floor(v), -qmax, qmax - 1)
    t64 = v.astype(np.float64) - k.astype(np.float64)
    cell = (v > -1) & (v < 0)
    assert cell.any() and (v >= 1).any() and (v <= -1).any() and ((v >= 0) & (v < 1)).any()
    assert np.array_equal(t64.astype(np.float32).astype(np.float64)[~cell], t64[~cell])
    assert np.abs(t64.astype(np.float32).astype(np.float64) - t64)[cell].max() <= 2.0 ** -25
    assert np.all(t64[live[:, None, :].repeat(50, 1)] >= -2.0 ** -16) and np.all(t64 <= 1.0 + 2.0 ** -16)
    ki = k.astype(np.int64)
    d = (cost[ki + 129] - cost[ki + 128]).astype(np.float32)
    want = (cost[ki + 128] + (t64.astype(np.float32) * d).astype(np.float32)).astype(np.float32)
    lv = live[:, None, :].repeat(50, 1)
    assert np.array_equal(terms[lv], want[lv])
    assert np.array_equal(slope[lv], (d * inv[:, None, :]).astype(np.float32)[lv])


# ---------------------------------------------------------------------------------------------------------------- the operator on CPU
@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("frames,hw,ld", SHAPES)
def test_cpu_operator_equals_the_reference_on_every_bit(frames, hw, ld, dtype, bits):
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    x = _data(frames, hw, ld, bits, seed=frames * 1000 + hw + bits)
    if dtype == "fp32" and ld > 6:
        x[:, :, 6:] = (x[:, :, 6:] * np.float32(1.0009765625) + np.float32(3e-5)).astype(np.float32)
    cost = _table(x, bits)
    ct = torch.from_numpy(cost)
    g = np.linspace(-1.5, 2.0, frames).astype(np.float32)
    if frames > 1:
        g[-1] = 0.0                                             # a negative entry and a zero
    for keep in _keeps(frames):
        xt = torch.from_numpy(x).to(dt).requires_grad_(True)
        kt = torch.from_numpy(keep).requires_grad_(True)
        terms, slope = rate_reference(x, keep, bits, cost)
        got_t, got_s = ops._rate_framework(xt.detach(), kt.detach(), float(qmax_of(bits)), ct)
        assert np.array_equal(got_t.numpy().view(np.uint32), terms.view(np.uint32)), keep.tolist()
        assert np.array_equal(got_s.numpy().view(np.uint32), slope.view(np.uint32)), keep.tolist()
        rate = ops.latent_rate(xt, kt, bits, ct)
        assert rate.shape == (frames,) and rate.dtype == torch.float32 and rate.requires_grad
        exact = terms.astype(np.float64).sum(axis=(1, 2))
        bound = hw * ld * 2.0 ** -24 * np.abs(terms).astype(np.float64).sum(axis=(1, 2))
        assert np.all(np.abs(rate.detach().numpy().astype(np.float64) - exact) <= bound), keep.tolist()
        rate.backward(torch.from_numpy(g))
        want = torch.from_numpy(np.where(((g == 0) | (keep == 0))[:, None, None], np.float32(0), g[:, None, None] * slope).astype(np.float32)).to(dt)
        assert xt.grad.dtype == dt and torch.equal(_bits_of(xt.grad), _bits_of(want)), keep.tolist()
        assert kt.grad is None
    x4 = torch.from_numpy(x).to(dt).reshape(1, frames, hw, ld)                     # leading dimensions pass through; keep as the models' (b, t, 1, 1)
    assert ops.latent_rate(x4, torch.ones(1, frames, 1, 1), bits, ct).shape == (1, frames)


def test_operator_refusals_before_any_work():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    x, keep, cost = torch.zeros(2, 4, 8), torch.ones(2), torch.zeros(256)
    for bad in (lambda: ops.latent_rate(x, keep, 1, cost), lambda: ops.latent_rate(x, keep, 9, cost),
                lambda: ops.latent_rate(x, torch.ones(3), 4, cost), lambda: ops.latent_rate(x, torch.ones(2, dtype=torch.int32), 4, cost),
                lambda: ops.latent_rate(x.transpose(0, 1), torch.ones(4), 4, cost), lambda: ops.latent_rate(x.half(), keep, 4, cost),
                lambda: ops.latent_rate(x, keep, 4, torch.zeros(255)), lambda: ops.latent_rate(x, keep, 4, cost.double()),
                lambda: ops.latent_rate(x, keep, 4, None), lambda: ops.latent_rate(x, keep.to("meta"), 4, cost),
                lambda: ops.latent_rate(x, keep, 4, cost.to("meta"))):
        with pytest.raises(VvaeError):
            bad()
    assert ops.latent_rate(torch.zeros(0, 4, 8), torch.ones(0), 4, cost).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- the cost table
@pytest.mark.parametrize("bits", [2, 4, 6, 8])
def test_cost_table_on_the_device_against_float64(bits):
    """loss.rate_cost_table against the definition evaluated in float64, within 1.5e-5 absolute: two logarithms of magnitude < 32 at <= 3 ulp
    each (OpenCL's bound for log2; 3 x 2^-19 = 5.7e-6) and the subtraction."""
    from video_vae_amd import loss as L
    qmax = qmax_of(bits)
    rng = np.random.default_rng(bits)
    live = np.abs(np.arange(256) - 128) <= qmax
    cases = [rng.integers(0, 40000, size=(16, 256)) * live * (rng.random((16, 256)) < 0.4), np.zeros((3, 256)), live[None] * 1,
             rng.integers(0, 2 ** 21, size=(2, 8, 256)) * live]
    for counts in cases:
        counts = counts.astype(np.int32)
        n = counts.reshape(-1, 256).sum(0).astype(np.float64)
        want = np.where(live, np.log2(n.sum() + (2 * qmax + 1) * 0.5) - np.log2(n + 0.5), 0.0)
        c = torch.from_numpy(counts).requires_grad_(False)
        got = L.rate_cost_table(c, bits)
        assert got.dtype == torch.float32 and got.shape == (256,) and not got.requires_grad
        assert np.abs(got.numpy().astype(np.float64) - want).max() <= 1.5e-5
        assert np.all(got.numpy()[~live] == 0)
        assert np.abs(rate_cost_reference(counts, bits).astype(np.float64) - want).max() <= 1.5e-5


# ---------------------------------------------------------------------------------------------------------------- loss and model
def _small(flavour, seed=2):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    from video_vae_amd import rl_model
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _cpu_model_and_loss(monkeypatch):
    """tests/test_quant_train_host.py's stand-ins for what runs on a GPU only (attention trunks, UNet, the reparameterisation kernel), plus
    one for the masked MSE / MAE kernel: the CPU forward and loss then run the model's and the loss's own code around them."""
    from einops import rearrange
    from video_vae_amd import model as M, ops
    monkeypatch.setattr(M.Encoder, "_features",
                        lambda self, x, mask: rearrange(x - 0.5, "b t (h p) (w q) c -> b t (h w) (p q c)", p=16, q=16).to(self.dtype))
    monkeypatch.setattr(M.Decoder, "forward", lambda self, x, mask, rngs, train=True: self.spatial_decompression(x))
    monkeypatch.setattr(ops, "reparameterise_kl", lambda mean, logvar, eps, mask_bt:
                        (mean.float() + eps.float() * torch.exp(0.5 * logvar.float()), torch.zeros(mean.shape[0])))

    def mse_mae(video, recon, mask_bt, video_div=1, partials=False):
        target = video.float().repeat_interleave(video_div, dim=0)
        diff = recon.float().reshape(target.shape[0], target.shape[1], -1) - target.reshape(target.shape[0], target.shape[1], -1)
        m = mask_bt[:, :, None]
        return (diff.square() * m).mean(dim=(1, 2)), (diff.abs() * m).mean(dim=(1, 2))
    monkeypatch.setattr(ops, "masked_mse_mae", mse_mae)


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_loss_adds_the_weighted_rate_and_nothing_without_the_key(flavour, monkeypatch):
    import video_vae_amd as V
    from video_vae_amd import loss as L, ops
    _cpu_model_and_loss(monkeypatch)
    m = _small(flavour)
    with torch.no_grad():
        m.encoder.selection_layer2.bias.fill_(-1.0)             # kept and dropped frames both occur
    b, t, bits, weight = 2, 4, 6, 0.01
    video = torch.rand((b, t, SMALL, SMALL, 3), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(b, t)
    mask[1, t - 1] = 0
    calls = []
    real = ops.latent_rate
    monkeypatch.setattr(ops, "latent_rate", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    fn = L.loss_fn if flavour == "rl" else L.loss_fn_plain

    def run(hparams):
        with torch.no_grad():
            return fn(m, video, L.compact_mask(mask), mask, V.Rngs(7), hparams)
    loss_q, aux_q = run(dict(L.HPARAMS, quant_bits=bits))
    assert not calls and "rate_bpp" not in aux_q and m._quant_rate is None and not m.latent_rate_on
    for off in ({"rate_weight": None}, {"rate_weight": 0}, {"rate_weight": 0.0}):
        loss_o, aux_o = run(dict(L.HPARAMS, quant_bits=bits, **off))
        assert not calls and torch.equal(loss_o, loss_q) and aux_o.keys() == aux_q.keys()
    loss_r, aux_r = run(dict(L.HPARAMS, quant_bits=bits, rate_weight=weight))
    assert len(calls) == 1 and m.latent_rate_on
    assert tuple(m._quant_rate.shape) == (2 * b if flavour == "rl" else b, t)   # left on the model, like _kl
    assert aux_r.keys() == aux_q.keys() | {"rate_bpp"}
    for k in aux_q:
        assert torch.equal(aux_r[k], aux_q[k]), k
    # the term, from the definitions: the gated latent the forward returned is the quantised one, so the unquantised one is rebuilt from a
    # run without the quantiser on the same seeds
    with torch.no_grad():
        m.latent_quant_bits, m.latent_rate_on = None, False
        plain = m(video, L.compact_mask(mask), V.Rngs(7), train=True)
    keep = (plain[3] if flavour == "rl" else plain[2]).reshape(-1).float().numpy()
    frames = keep.size
    comp = plain[1].float().reshape(frames, 4, 96).numpy()
    assert 0 < np.count_nonzero(keep) < frames
    q = quantise_reference(comp[keep != 0], bits)[0]
    terms, _ = rate_reference(comp, keep, bits, rate_cost_reference(code_counts(q), bits))
    rate = terms.astype(np.float64).sum(axis=(1, 2)).reshape(-1, t)
    om = mask.numpy().repeat(2, axis=0) if flavour == "rl" else mask.numpy()
    want = float(((rate * om).sum(1) / (SMALL * SMALL * np.maximum(om.sum(1), 1.0))).mean())
    got = float(aux_r["rate_bpp"])
    print(f"{flavour}: rate_bpp {got!r}, from the reference in float64 {want!r}; loss {float(loss_q)!r} -> {float(loss_r)!r}")
    assert want > 0 and abs(got - want) <= 1e-4 * want          # fp32 sums of 384 terms per frame and a table at 1.5e-5: far inside
    assert torch.equal(loss_r, loss_q + weight * aux_r["rate_bpp"])
    # switching off again: the model launches nothing for the rate and the numbers are those of before
    loss_b, aux_b = run(dict(L.HPARAMS, quant_bits=bits))
    assert len(calls) == 1 and torch.equal(loss_b, loss_q) and "rate_bpp" not in aux_b and m._quant_rate is None
    for bad in (dict(L.HPARAMS, rate_weight=weight), dict(L.HPARAMS, quant_bits=None, rate_weight=weight),
                dict(L.HPARAMS, quant_bits=bits, rate_weight=-1.0)):
        with pytest.raises(ValueError):
            run(bad)


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_rate_gradient_reaches_the_encoder(flavour, monkeypatch):
    """With the decoder's gradient the same (straight-through), the encoder's gradients with the rate term differ from those without."""
    import video_vae_amd as V
    from video_vae_amd import loss as L
    _cpu_model_and_loss(monkeypatch)
    m = _small(flavour)
    video = torch.rand((2, 4, SMALL, SMALL, 3), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(2, 4)
    fn = L.loss_fn if flavour == "rl" else L.loss_fn_plain
    grads = []
    for extra in ({}, {"rate_weight": 0.01}):
        m.zero_grad()
        loss, _ = fn(m, video, L.compact_mask(mask), mask, V.Rngs(7), dict(L.HPARAMS, quant_bits=6, **extra))
        loss.backward()
        grads.append({k: p.grad.clone() for k, p in m.encoder.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and "spatial_compression.kernel" in grads[0]
    assert all(bool(torch.isfinite(g).all()) for g in grads[1].values())
    assert not torch.equal(grads[0]["spatial_compression.kernel"], grads[1]["spatial_compression.kernel"])


# ---------------------------------------------------------------------------------------------------------------- what the term is for
@pytest.mark.parametrize("bits", [4, 6, 8])
def test_descent_on_the_rate_lowers_the_entropy_of_the_codes(bits):
    """50 plain gradient steps of 0.02 on the sum of ops.latent_rate over free standard-normal values, the table rebuilt from the codes'
    histogram every step (loss.rate_cost_table): the zeroth-order entropy of the codes ends at no more than 2/3 of where it started.  The
    reference alone reaches 0.33, 0.43 and 0.40 of the start at 4, 6 and 8 bits."""
    from video_vae_amd import loss as L, ops
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((4, 64, 16)).astype(np.float32))
    keep = torch.ones(4)

    def counts_of(t):
        return code_counts(quantise_reference(t.numpy(), bits)[0])
    start = entropy_bits(counts_of(x))
    for i in range(50):
        counts = counts_of(x)
        cost = L.rate_cost_table(torch.from_numpy(counts.astype(np.int32)), bits)
        leaf = x.clone().requires_grad_(True)
        rate = ops.latent_rate(leaf, keep, bits, cost)
        if i == 0:
            relaxed = float(rate.detach().sum()) / x.numel()
            assert abs(relaxed - start) <= 0.05, (relaxed, start)                   # the relaxed rate starts at the hard entropy
        rate.sum().backward()
        x = x - 0.02 * leaf.grad
    end = entropy_bits(counts_of(x))
    print(f"bits {bits}: entropy {start:.3f} -> {end:.3f} ({end / start:.3f} of the start)")
    assert end <= start * 2 / 3


# ---------------------------------------------------------------------------------------------------------------- driver and ABI
def test_train_flags():
    from video_vae_amd import train
    assert train.parse_args([]).rate_weight is None
    a = train.parse_args(["--quantise-bits", "6", "--quantise-after", "4", "--rate-weight", "0.01"])
    assert (a.quantise_bits, a.quantise_after, a.rate_weight) == (6, 4, 0.01)
    assert train.parse_args(["--quantise-bits", "6", "--rate-weight", "0"]).rate_weight == 0.0
    for bad in (["--rate-weight", "0.01"], ["--quantise-bits", "6", "--rate-weight", "-1"], ["--quantise-bits", "6", "--rate-weight", "nan"],
                ["--quantise-after", "4", "--rate-weight", "0.01"]):
        with pytest.raises(SystemExit):
            train.parse_args(bad)


def test_header_declares_and_library_exports_the_entries():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    assert "vvae_latent_rate" in protos and len(protos["vvae_latent_rate"][1]) == 10
    assert "vvae_latent_rate_grad" in protos and len(protos["vvae_latent_rate_grad"][1]) == 11
    assert len(protos["vvae_latent_fake_quant"][1]) == 10                           # the existing entry keeps its signature
    assert getattr(lib(), "vvae_latent_rate") is not None and getattr(lib(), "vvae_latent_rate_grad") is not None
