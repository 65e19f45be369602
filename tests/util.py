"""Shared helpers for the parity tests (tests only)."""
import numpy as np
import torch

RTOL, ATOL = 1e-3, 1e-4          # fp32 parity bar of BASELINE.json:north_star


def assert_close(got, want, rtol=RTOL, atol=ATOL, what=""):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    bad = err > tol
    if bad.any():
        i = (err - tol).argmax()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outside rtol={rtol} atol={atol}; "
                             f"worst |err|={float(err.flatten()[i]):.3e} at want={float(want.flatten()[i]):.3e}, "
                             f"max|want|={float(want.abs().max()):.3e}")


def assert_close_scaled(got, want, rel=1e-3, what="", floor=0.0):
    """Tolerance relative to the tensor's scale: for gradients whose magnitude is far from 1.

    ``floor``: a lower bound for that scale, for gradients that are exactly zero in exact arithmetic and pure
    rounding noise in floating point (a conv bias in front of a GroupNorm with one channel per group).
    """
    want_c = want.detach().float().cpu()
    scale = max(float(want_c.abs().max()), floor)
    assert_close(got, want, rtol=rel, atol=rel * max(scale, 1e-30), what=what)


def grad_floor(name, ref_grads):
    """Scale floor for the gradient of parameter ``name``: the kernel-gradient scale of the same conv for its bias."""
    if name.endswith("conv.bias"):
        return float(ref_grads[name[:-4] + "kernel"].abs().max())
    return 0.0


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ------------------------------------------------------------------------------------------- exact-arithmetic parity (test_gpu_exact.py)
EXACT_LIMIT = 2 ** 24            # integers below this magnitude add exactly in fp32, in any order


def ints(shape, seed, lo, hi, density=1.0):
    """Seeded integer-valued fp32 tensor, uniform in {lo ... hi}; each entry is zeroed with probability 1 - density."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int8 if -128 <= lo and hi <= 127 else torch.int32).float()
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density)
    return v


def assert_representable(ref64, dtype, partial_bound):
    """Validity of an exact-arithmetic reference, checked before any GPU result is looked at: every value of ``ref64`` is an integer
    that survives the round trip through the output ``dtype`` (bf16: integers up to 256, and the even ones a little above; fp32:
    below 2^24), and no partial sum of the product can leave the exact range of fp32 (``partial_bound``: number of terms x max|a| x
    max|b|, or a tighter |A|.|B|).  A condition on the INPUTS, not a measurement: no element is ever exempted -- a failure here means
    the value range or the density of the test's operands has to come down."""
    assert partial_bound < EXACT_LIMIT, f"a partial sum may reach {partial_bound} >= 2^24: fp32 accumulation is no longer order-free"
    r = ref64.detach()                                        # on whatever device the caller holds it: elementwise torch either way
    assert r.dtype in (torch.float64, torch.float32), r.dtype
    assert bool((r == r.round()).all()), "reference is not integer-valued"
    top = float(r.abs().max()) if r.numel() else 0.0
    assert top < EXACT_LIMIT, f"max |reference| = {top} >= 2^24"
    bad = r.to(dtype).to(r.dtype) != r
    nbad = int(bad.sum())
    assert nbad == 0, f"{nbad}/{r.numel()} reference values do not survive {dtype} (max |reference| = {top}): narrow the operands"


def assert_exact(got, want64, what):
    """``got`` equals the high-precision reference cast to got's dtype, element for element and with zero tolerance (the two zeros
    of floating point count as the same integer; a NaN never matches).  Reports how many elements differ, and where the first ones
    are -- the indices name the tile or the edge that is wrong."""
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    want = want64.detach().to(got.device).to(got.dtype)
    bad = ~(got.detach() == want)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()[:8].cpu()
        rows_ = [f"{tuple(i.tolist())}: got {float(got[tuple(i)])} want {float(want[tuple(i)])}" for i in idx]
        last = tuple(bad.nonzero()[-1].tolist())
        raise AssertionError(f"{what}: {nbad}/{bad.numel()} elements differ from the exact reference, shape {tuple(got.shape)}; first at "
                             + "; ".join(rows_) + f"; last at {last}")


# ------------------------------------------------------------------------------------------- exact softmax families (test_gpu_attn_exact.py)
def assert_rounded(got, want64, rel, what):
    """|got - want| <= rel * |want| element for element, and ``got`` exactly 0 wherever ``want`` is 0.  ``rel`` is a number or a tensor
    that broadcasts against ``want64`` (0 where the value is a number of got's dtype and no rounding is allowed, 2^-7 where a bf16
    probability and a bf16 output were each rounded once).  The bound scales with the value itself, so no absolute slack can hide a
    dropped or doubled term.  A NaN never passes."""
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    g = got.detach().double().cpu()
    w = want64.detach().double().cpu()
    tol = torch.as_tensor(rel, dtype=torch.float64).cpu() * w.abs()
    err = (g - w).abs()
    bad = ~(err <= tol)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()[:8]
        rows_ = [f"{tuple(i.tolist())}: got {float(g[tuple(i)])!r} want {float(w[tuple(i)])!r}" for i in idx]
        zeros = int((bad & (w == 0)).sum())
        raise AssertionError(f"{what}: {nbad}/{bad.numel()} elements outside rel * |want| ({zeros} of them where the reference is exactly 0), "
                             f"shape {tuple(got.shape)}; first at " + "; ".join(rows_) + f"; last at {tuple(bad.nonzero()[-1].tolist())}")
    return float((err / w.abs().clamp_min(1e-300))[w != 0].max()) if bool((w != 0).any()) else 0.0


def assert_abs(got, want64, atol, what):
    """|got - want| <= atol element for element (log-sum-exp rows: the bound is a few spacings of fp32 at the value's size)."""
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    err = (got.detach().double().cpu() - want64.detach().double().cpu()).abs()
    bad = ~(err <= atol)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements off by more than {atol}; first at {i}: "
                             f"got {float(got[i])!r} want {float(want64[i])!r}; worst {float(err[~err.isnan()].max()) if bool((~err.isnan()).any()) else float('nan'):.3e}")
    return float(err.max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------- the range coder (test_gpu_entropy*.py)
def coded_garbage(frames, cap, dev):
    """An ``out=`` for the rANS encoders in the capacity layout, full of values that no encoder writes."""
    from video_vae_amd.entropy import CodedFrames
    return CodedFrames(torch.from_numpy(np.full((frames, cap), 0x5a5a, dtype=np.uint16)).to(dev),
                       torch.full((frames,), -7, dtype=torch.int32, device=dev),
                       torch.from_numpy(np.full((frames, 64), 0xdeadbeef, dtype=np.uint32)).to(dev))


def capacity_offsets(n_words, cap, dev):
    """Where frame f's stream starts in the capacity layout: the last n_words[f] entries of its row of ``cap`` words."""
    return torch.arange(n_words.shape[0], device=dev, dtype=torch.int64) * cap + cap - n_words.to(torch.int64)
