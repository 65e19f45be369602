"""Shared helpers for the parity tests (tests only)."""
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
