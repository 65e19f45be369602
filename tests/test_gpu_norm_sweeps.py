"""LayerNorm and GroupNorm + SiLU past one sweep of their grids, against fp64, with one family of inputs whose statistics are exact.

Both kernel families are persistent streams: a capped grid walks the rows (layernorm.hip) or the voxels (gn_silu.hip) in sweeps, and a
workgroup carries column sums across its sweeps.  The other direct tests stay inside the first sweep.  Here the shapes alone reach the
loops (no tuning hook is touched), and every case asserts the regime it means to be in, from mirrors of ln_pick / ln_blocks / pick_vpb
that are held against what the library reports, so a retuning fails loudly instead of shrinking the coverage.

  * Family G, Gaussian: the inputs of test_gpu_ops.py, rounded to the case dtype; the reference is the fp64 closed form on the CPU
    (F.layer_norm / F.group_norm + SiLU in double, gradients by autograd) at the bars test_layer_norm / test_group_norm_silu use.  A
    wrong row or voxel in y or dx is wrong by O(1).  "G8" is the same with a mean of 8 and unit spread (the fast variance and the
    folded bb = beta - mean * a, k2 constants are where an offset costs bits).

  * Family B, balanced rows: a row (LayerNorm) or a (sample, group) slab (GroupNorm) is m + a * s, s in {+1, -1} with exactly half of
    each in a seeded order (a slab of odd size carries one s = 0), m in {0, 3, -2}, a in {1, 2, 0.5}.  Sum x and sum x^2 are small
    dyadics: the mean is exactly m, the fast variance exactly a^2 (times (M - 1) / M for an odd slab), xhat = s * rho with
    rho = a / sqrt(var + eps).  dy is small integers.
      LayerNorm: gamma in {1, 2, 0.5, -1}, beta in {-6, -4, 4, 6}: no output is 0 and s * gamma + beta is a bf16 number.
        y bf16: zero tolerance against s * gamma + beta (a wrong row flips signs: the defect is at least 1).
        y fp32: absolute 1e-5 against the fp64 value (|y| <= 8, where fp32 is spaced 9.5e-7; rsqrt and three roundings).
        dbias:  zero tolerance (integers of magnitude <= 2 rows < 2^24 add exactly in fp32 in any order: partial rows and fold alike).
        dscale: |err| <= 2^-20 sum_r |dy_rc| against rho64 * sum_r(dy s): 16 times the worst case of an fp32 accumulation of terms
                that are each good to an ulp.  The builder asserts that this is below half of min(rho), i.e. half of what ONE row
                with dy != 0 moves the sum by, before any GPU result is looked at.
        dx:     fp64 reference at Family G's bar.
      GroupNorm: gamma and beta are drawn so that both values z takes per (sample, channel) lie in [-0.5, 3], where |silu'| >= 0.26.
        gn_stats_raw: zero tolerance on both sums (fp64 sums of per-workgroup fp32 partials that are exact dyadics).
        dgamma, dbeta: z takes the values z+ / z- (/ z0), so silu'(z) takes the constants d+ / d- (/ d0); the references are
                sum_n(d+ K+ + d- K- + d0 K0) and sum_n rho (d+ K+ - d- K-) with integer K = sums of dy over the voxels of each sign, in
                fp64.  Bound 2^-19 sum|dy| max|d|: the fp32 accumulation as above, and one more bit for the kernel's sigmoid
                (v_exp_f32 and v_rcp_f32, an ulp each; the error of d at a given z is the same for every voxel, so it does not
                average out).  The builder thins dy until the bound is below half the smallest single-voxel defect and asserts it.
        y, dx:  fp64 reference at the project's bars.

No family asserts "mostly": the share of elements a check may leave out is zero.

Every builder validates its case on the CPU before a GPU result is looked at: representability, the "bound < half a defect" conditions,
and a CPU result in the case's dtype passing the very assertions the GPU result meets.  For y of LayerNorm that CPU result is
oracle.nn.layer_norm; the gradients, and all of GroupNorm + SiLU, come from the kernels' own closed form in fp32 (cpu_ln, cpu_gn): the
oracle's GroupNorm rounds z to bf16 between the norm and the SiLU, which the fused kernel does not, and 2^-9 of z is far outside the
2^-19 bound.  tests/test_host.py runs the builders without a GPU (HOST_CHECKS) and feeds the assertions CPU results with one defect
each (DEFECT_CHECKS): every one of them must raise.

Each GPU test prints the largest error-to-bound ratio it saw per route (FIGURE lines; NOTES.md, "norm sweeps").
"""
import functools
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import nn as O
from util import assert_exact, assert_representable, ints, rnd

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
FIGURES = {}                             # (route, what) -> largest error / bound seen (printed by the GPU tests)
Y_F32_ABS = 1e-5                         # Family B, LayerNorm y in fp32
LN_U, GN_U = 2.0 ** -20, 2.0 ** -19      # Family B column sums, see the module docstring


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31 - 1000)


def _q(x, dtype):
    return x.to(dtype).float()


def _note(route, what, value):
    FIGURES[(route, what)] = max(FIGURES.get((route, what), 0.0), float(value))


@pytest.fixture(autouse=True)
def _fresh_figures():
    FIGURES.clear()                      # each test reports what it saw itself


def _report(route):
    for (r, what), v in sorted(FIGURES.items()):
        if r == route:
            print(f"FIGURE {route}: {what}: error / bound = {v:.3e}")


def _within(got, want64, tol, what, route, name):
    """|got - want| <= tol element for element (tol a number or a tensor); a NaN never passes.  Notes max(err / tol) first."""
    assert tuple(got.shape) == tuple(want64.shape), (what, name, tuple(got.shape), tuple(want64.shape))
    err = (got.detach().double().cpu() - want64.double()).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand(err.shape)
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), (err != 0).double() * float("inf")).nan_to_num(nan=0.0, posinf=float("inf"))
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    _note(route, name, worst)
    bad = ~(err <= tol)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        raise AssertionError(f"{what}: {name}: {nbad}/{bad.numel()} elements outside the bound, worst error / bound {worst:.3e}; first at {i}: "
                             f"got {float(got[i])!r} want {float(want64[i])!r} bound {float(tol[i]):.3e}; last at {tuple(idx[-1].tolist())}")


def _bar(got, want64, rtol, atol, what, route, name):
    """util.assert_close's bar, atol + rtol |want|, against an fp64 reference."""
    _within(got, want64, atol + rtol * want64.double().abs(), what, route, name)


def _bar_scaled(got, want64, rel, what, route, name):
    """util.assert_close_scaled's bar: rel (max|want| + |want|)."""
    _bar(got, want64, rel, rel * max(float(want64.abs().max()), 1e-30), what, route, name)


def _exact(got, want64, what, name):
    assert_exact(got.detach().cpu(), want64, f"{what}: {name}")


def _finite(res, what):
    for name, x in res.items():
        bad = int((~torch.isfinite(x.float())).sum())
        assert bad == 0, f"{what}: {name}: {bad}/{x.numel()} elements are not finite"


def balanced(slabs, m_, seed):
    """(slabs, m_) of +1 / -1, exactly m_ // 2 of each per slab in a seeded order (one 0 if m_ is odd); m and a per slab."""
    g = torch.Generator().manual_seed(seed)
    base = torch.cat([torch.ones(m_ // 2), -torch.ones(m_ // 2), torch.zeros(m_ % 2)])
    s = base[torch.rand((slabs, m_), generator=g).argsort(1)]
    m = torch.tensor([0.0, 3.0, -2.0])[torch.randint(0, 3, (slabs,), generator=g)][:, None]
    a = torch.tensor([1.0, 2.0, 0.5])[torch.randint(0, 3, (slabs,), generator=g)][:, None]
    assert bool((s.sum(1) == 0).all()) and bool(((s != 0).sum(1) == m_ - m_ % 2).all())
    return s, m, a


# =========================================================================================== LayerNorm: the dispatch, mirrored
LN_BW, LN_BWD_CAP = 8, 384               # layernorm.hip: LN_BW (waves per backward workgroup), LN_BWD_CAP
LN_FWD_CAP = {BF16: 1024, F32: 2048}     # LN_FWD_CAP (bf16), the literal of the fp32 branch of vvae_layernorm_fwd


def ln_pick(c, dtype):
    v = 8 if dtype == BF16 else 4
    assert c % v == 0
    nv, lpr = c // v, 8
    while lpr < 64 and (nv + lpr - 1) // lpr > 4:
        lpr *= 2
    vpl = (nv + lpr - 1) // lpr
    assert vpl <= 4
    return lpr, vpl


def ln_sweeps(c, dtype):
    """Rows one sweep of the forward / of the backward grid covers once it is capped, and rows per wave-iteration."""
    rpw = 64 // ln_pick(c, dtype)[0]
    return LN_FWD_CAP[dtype] * 4 * rpw, LN_BWD_CAP * LN_BW * rpw, rpw


# =========================================================================================== LayerNorm: cases
HEAD_DIM = 64


@functools.lru_cache(maxsize=1)
def ln_case(family, rows, c, dtype, heads=0):
    """heads > 0: the rows are the per-head k slices of a fused (tokens, 3 heads 64) buffer, rows = tokens * heads."""
    assert heads == 0 or (c == HEAD_DIM and rows % heads == 0)
    k = types.SimpleNamespace()
    k.family, k.rows, k.c, k.dtype, k.heads = family, rows, c, dtype, heads
    seed = _seed("ln", family, rows, c, str(dtype), heads)
    if family == "B":
        k.s, k.m, k.a = balanced(rows, c, seed)
        k.x = k.m + k.a * k.s
        g = torch.Generator().manual_seed(seed + 1)
        k.gamma = torch.tensor([1.0, 2.0, 0.5, -1.0])[torch.randint(0, 4, (c,), generator=g)]
        k.beta = torch.tensor([-6.0, -4.0, 4.0, 6.0])[torch.randint(0, 4, (c,), generator=g)]
        k.dy = ints((rows, c), seed + 2, -2, 2)
        k.dskip = ints((rows, c), seed + 3, -2, 2)
        k.o = ints((rows, c), seed + 4, -1, 1)
        k.skip = k.x - k.o
    else:
        k.skip = _q(rnd((rows, c), seed) * 1.3 + 0.2, dtype) if family == "G" else _q(rnd((rows, c), seed) + 8.0, dtype)
        k.o = _q(rnd((rows, c), seed + 4, 0.3), dtype)
        k.x = _q(k.skip + k.o, dtype)                                    # what the add route normalises; every route shares it
        k.gamma, k.beta = 1 + 0.2 * rnd((c,), seed + 1), 0.1 * rnd((c,), seed + 5)
        k.dy, k.dskip = _q(rnd((rows, c), seed + 2), dtype), _q(rnd((rows, c), seed + 3), dtype)
    for name in ("x", "skip", "o", "dy", "dskip"):
        t = getattr(k, name)
        assert bool((_q(t, dtype) == t).all()), f"{name} is no {dtype} tensor"
    assert bool((_q(k.skip + k.o, dtype) == k.x).all())
    if heads:
        hd = heads * HEAD_DIM
        k.qkv = _q(rnd((rows // heads, 3 * hd), seed + 6) * 1.3 + 0.2, dtype)
        k.qkv[:, hd:2 * hd] = k.x.reshape(rows // heads, hd)
    x64 = k.x.double().requires_grad_(True)
    g64, b64 = k.gamma.double().requires_grad_(True), k.beta.double().requires_grad_(True)
    y64 = F.layer_norm(x64, (c,), g64, b64, EPS)
    y64.backward(k.dy.double())
    k.y, k.dx, k.dscale, k.dbias = y64.detach(), x64.grad, g64.grad, b64.grad
    if family == "B":
        rho = k.a.double() / torch.sqrt(k.a.double() ** 2 + EPS)
        assert float((1 - rho).abs().max()) < 2e-6
        k.y_exact = (k.s * k.gamma + k.beta).double()
        assert bool((k.y_exact != 0).all()) and float((k.y_exact - k.y).abs().max()) < 5e-6
        if dtype == BF16:
            assert bool((k.y_exact.to(BF16).double() == k.y_exact).all())
        k.dbias_exact = k.dy.double().sum(0)
        assert_representable(k.dbias_exact, F32, 2 * rows)
        k.dscale_ref = (rho * k.dy.double() * k.s.double()).sum(0)
        k.dscale_bound = LN_U * k.dy.double().abs().sum(0)
        assert float((k.dscale_ref - k.dscale).abs().max()) <= 1e-9 * float(k.dscale.abs().max())
        assert float(k.dscale_bound.max()) < 0.5 * float(rho.min()), "thin dy: the dscale bound no longer separates one row"
    assert bool(torch.isfinite(k.dx).all())
    res = cpu_ln(k, "strided" if heads else "plain")
    check_ln(k, res, "cpu")
    check_ln(k, dict(res, y=O.layer_norm(k.x, k.gamma, k.beta, dtype)), "oracle")
    return k


def _gather_rows(flat, base, rows, c, inner, outer_pitch, inner_pitch):
    r = torch.arange(rows)
    off = (base + (r // inner) * outer_pitch + (r % inner) * inner_pitch) % (flat.numel() - c)
    return flat[off[:, None] + torch.arange(c)[None, :]]


def cpu_ln(k, route, defect=None):
    """layernorm_fwd_kernel / layernorm_bwd_kernel in fp32 torch on the CPU, rounded to the case dtype where the kernels round; with
    ``defect`` it makes one of the mistakes a sweeping kernel makes: "row-dropped" / "row-doubled" (the last row, in dscale and dbias),
    "tail-unwritten" (y and dx of the last wave-iteration), "neighbour-mean", "pitches-swapped" (the strided route)."""
    dt, c, rows = k.dtype, k.c, k.rows
    x = k.x
    if route == "strided":
        hd = k.heads * HEAD_DIM
        pitches = (HEAD_DIM, 3 * hd) if defect == "pitches-swapped" else (3 * hd, HEAD_DIM)
        x = _gather_rows(k.qkv.flatten(), hd, rows, c, k.heads, *pitches)
        assert defect is not None or torch.equal(x, k.x)
    mean = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + EPS)
    if defect == "neighbour-mean":                                       # a row whose neighbour has another mean
        r = int(((mean[:-1] - mean[1:]).abs() > 0.01).nonzero()[0, 0])
        mean = mean.clone()
        mean[r] = mean[r + 1]
    y = _q((x - mean) * (rstd * k.gamma) + k.beta, dt)
    xh = (x - mean) * rstd
    w = torch.ones((rows, 1))
    if defect in ("row-dropped", "row-doubled"):
        w[rows - 1] = 0.0 if defect == "row-dropped" else 2.0
    dscale = (k.dy * xh * w).double().sum(0).float()
    dbias = (k.dy * w).double().sum(0).float()
    gg = k.dy * k.gamma
    s1, s2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    dx = rstd * (gg - s1 - xh * s2)
    if route in ("fork", "add"):
        dx = _q(dx, dt) + k.dskip
    dx = _q(dx, dt)
    if defect == "tail-unwritten":                                       # the last wave-iteration: its rows keep what the buffer held
        r0 = (rows - 1) // ln_sweeps(c, dt)[2] * ln_sweeps(c, dt)[2]
        y[r0:], dx[r0:] = 0.0, 0.0
    return {"y": y, "dx": dx, "dscale": dscale, "dbias": dbias}


def check_ln(k, res, route):
    """Every assertion of a case on {y, dx (rows, C); dscale, dbias (C)} of one route: plain, fork, add, strided."""
    what = f"{route} {k.family} {k.dtype} (rows {k.rows}, C {k.c}, heads {k.heads})"
    _finite(res, what)
    r, ya = (1e-3, 1e-4) if k.dtype == F32 else (2e-2, 2e-2)            # test_gpu_ops.py::test_layer_norm
    dx64 = k.dx + k.dskip.double() if route.split("-")[-1] in ("fork", "add") else k.dx     # "cpu-fork": the CPU twin of a route
    if k.family != "B":
        _bar(res["y"], k.y, r, ya, what, route, f"{k.family} y")
    elif k.dtype == BF16:
        _exact(res["y"], k.y_exact, what, "y")
    else:
        _within(res["y"], k.y, Y_F32_ABS, what, route, "B y fp32")
    _bar_scaled(res["dx"], dx64, r, what, route, f"{k.family} dx")
    if k.family == "B":
        _exact(res["dbias"], k.dbias_exact, what, "dbias")
        _within(res["dscale"], k.dscale_ref, k.dscale_bound, what, route, "B dscale")
    else:
        _bar_scaled(res["dscale"], k.dscale, r, what, route, f"{k.family} dscale")
        _bar_scaled(res["dbias"], k.dbias, r, what, route, f"{k.family} dbias")


# dtype, C, rows: the smallest that give both kernels a second sweep and a ragged last wave-iteration (fwd sweep, bwd sweep):
LN_SWEEPS = [(BF16, 768, 16387),         # 8192 x 2 + 3, 6144 x 2.7
             (BF16, 64, 65549),          # 32768 x 2 + 13, 24576 x 2.7
             (BF16, 40, 32777),          # one sweep + 9, 24576 x 1.3; lanes 5..7 of each row group idle
             (F32, 768, 16387),          # 8192 x 2 + 3, 3072 x 5.3
             (F32, 1024, 8197)]          # one sweep + 5, 3072 x 2.7; 64 lanes per row, 4 vectors per lane
LN_CAP_EDGE = [(BF16, 768, r) for r in (6143, 6144, 6145)]               # the backward cap boundary
LN_MEAN8 = (F32, 768, 16387)
LN_STRIDED = [(BF16, 8, 4100), (F32, 8, 4100),                           # 32800 rows: bf16 past one sweep of both kernels, fp32 of the backward
              (F32, 8, 8201)]                                            # 65608 rows: past the 65536 of the fp32 forward sweep as well
LN_ROUTES = ("plain", "fork", "add")


def _ln_host_cases():
    cs = [(f"ln-{fam}-{dt}-C{c}-rows{r}", functools.partial(ln_case, fam, r, c, dt)) for fam in ("G", "B") for dt, c, r in LN_SWEEPS + LN_CAP_EDGE]
    cs += [(f"ln-G8-{LN_MEAN8}", functools.partial(ln_case, "G8", LN_MEAN8[2], LN_MEAN8[1], LN_MEAN8[0]))]
    cs += [(f"ln-strided-{fam}-{dt}-tokens{t}", functools.partial(ln_case, fam, t * h, HEAD_DIM, dt, h)) for fam in ("G", "B") for dt, h, t in LN_STRIDED]
    return cs


def _ln_routes_on_cpu(make):
    k = make()
    for route in ("fork", "add"):                                        # the builder itself checked the plain (or strided) route
        check_ln(k, cpu_ln(k, route), "cpu-" + route)


def _ln_defect_check(make, route, defect, first):
    k = make()
    if defect is None:
        check_ln(k, cpu_ln(k, route), "cpu-" + route)
        return
    with pytest.raises(AssertionError, match=rf"\): {first}: \d+/\d+ "):
        check_ln(k, cpu_ln(k, route, defect), "cpu-" + route)


def _ln_defect_checks():
    """Small cases (rows 403 = 50 wave-iterations of 8 rows and a ragged one; 51 tokens of 8 heads), each defect fed to the assertions
    it has to trip.  The dropped and the doubled row go to Family B alone: that a scaled bar may not see them is why Family B exists."""
    out = []
    for dt in (BF16, F32):
        for fam in ("B", "G"):
            mk = functools.partial(ln_case, fam, 403, 64, dt)
            mks = functools.partial(ln_case, fam, 51 * 8, HEAD_DIM, dt, 8)
            ny = f"{fam} y" if fam == "G" else "y" if dt == BF16 else "B y fp32"
            out.append((f"ln-{fam}-{dt}-clean", functools.partial(_ln_defect_check, mk, "plain", None, None)))
            out.append((f"ln-{fam}-{dt}-tail-unwritten", functools.partial(_ln_defect_check, mk, "plain", "tail-unwritten", ny)))
            out.append((f"ln-{fam}-{dt}-neighbour-mean", functools.partial(_ln_defect_check, mk, "plain", "neighbour-mean", ny)))
            out.append((f"ln-{fam}-{dt}-pitches-swapped", functools.partial(_ln_defect_check, mks, "strided", "pitches-swapped", ny)))
            if fam == "B":
                for route in ("plain", "fork"):
                    out.append((f"ln-B-{dt}-{route}-row-dropped", functools.partial(_ln_defect_check, mk, route, "row-dropped", "dbias")))
                    out.append((f"ln-B-{dt}-{route}-row-doubled", functools.partial(_ln_defect_check, mk, route, "row-doubled", "dbias")))
    return out


def _ln_dscale_alone_sees_a_row():
    """dbias fires first in check_ln; the dscale bound on its own must see one row as well (dbias put right by hand)."""
    k = ln_case("B", 403, 64, F32)
    for defect in ("row-dropped", "row-doubled"):
        res = dict(cpu_ln(k, "plain", defect), dbias=k.dbias_exact.float())
        with pytest.raises(AssertionError, match=r"\): B dscale: \d+/\d+ "):
            check_ln(k, res, "cpu")


# =========================================================================================== GroupNorm + SiLU: the dispatch, mirrored
def pick_vpb(s, n, total_blocks):
    """gn_silu.hip: voxels per workgroup.  1024 workgroups for the reducing kernels (stats, backward reduce), 4096 for the streaming ones."""
    want = max(1, total_blocks // max(n, 1))
    return max(128, (s + want - 1) // want)


GN_Z_LO, GN_Z_HI, GN_D_MIN = -0.5, 3.0, 0.26
# (gamma, beta) with -0.5 < beta - |gamma| rho and beta + |gamma| rho < 3 for rho up to 1.001
GN_AFFINE = [(1.0, 0.75), (1.0, 1.5), (1.0, 1.75), (0.5, 0.25), (0.5, 1.25), (0.5, 2.25), (-1.0, 1.0), (-1.0, 1.75), (1.5, 1.125), (1.5, 1.25)]


def _dsilu64(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


@functools.lru_cache(maxsize=1)
def gn_case(family, shape, groups, dtype):
    k = types.SimpleNamespace()
    n, c = shape[0], shape[-1]
    s_ = shape[1] * shape[2] * shape[3]
    cpg = c // groups
    k.family, k.shape, k.groups, k.dtype, k.n, k.s_, k.c, k.cpg = family, shape, groups, dtype, n, s_, c, cpg
    k.vpb_r, k.vpb_s = pick_vpb(s_, n, 1024), pick_vpb(s_, n, 4096)
    k.nblk = (s_ + k.vpb_r - 1) // k.vpb_r
    seed = _seed("gn", family, shape, groups, str(dtype))
    m_ = s_ * cpg
    if family == "B":
        sg, m, a = balanced(n * groups, m_, seed)
        to_x = lambda t: t.reshape(n, groups, s_, cpg).permute(0, 2, 1, 3).reshape(n, s_, c).contiguous()
        k.s = to_x(sg)
        k.x = to_x(m + a * sg)
        g = torch.Generator().manual_seed(seed + 1)
        pick = torch.tensor(GN_AFFINE)[torch.randint(0, len(GN_AFFINE), (c,), generator=g)]
        k.gamma, k.beta = pick[:, 0].contiguous(), pick[:, 1].contiguous()
        k.density = min(1.0, 45000.0 / (1.2 * n * s_))                   # sum|dy| per channel about 45000: the bound about 0.1
        k.dy = ints((n, s_, c), seed + 2, -2, 2, k.density)
    else:
        k.x = _q(rnd((n, s_, c), seed) * 1.5 + 0.3, dtype) if family == "G" else _q(rnd((n, s_, c), seed) + 8.0, dtype)
        k.gamma, k.beta = 1 + 0.2 * rnd((c,), seed + 1), 0.1 * rnd((c,), seed + 3)
        k.dy = _q(rnd((n, s_, c), seed + 2), dtype)
    assert bool((_q(k.x, dtype) == k.x).all()) and bool((_q(k.dy, dtype) == k.dy).all())
    xg = k.x.double().reshape(n, s_, groups, cpg)
    k.sums = torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1)    # (n, G, 2), fp64
    k.sums_abs = torch.stack([xg.abs().sum((1, 3)), (xg * xg).sum((1, 3))], -1)
    x64 = k.x.double().requires_grad_(True)
    g64, b64 = k.gamma.double().requires_grad_(True), k.beta.double().requires_grad_(True)
    y64 = F.silu(F.group_norm(x64.permute(0, 2, 1), groups, g64, b64, EPS)).permute(0, 2, 1)
    y64.backward(k.dy.double())
    k.y, k.dx, k.dgamma, k.dbeta = y64.detach(), x64.grad, g64.grad, b64.grad
    if family == "B":
        pad = k.nblk * k.vpb_r - s_                                      # the per-workgroup fp32 partials are exact dyadics: 4 x them integers
        xp = F.pad(xg, (0, 0, 0, 0, 0, pad)).reshape(n, k.nblk, k.vpb_r, groups, cpg)
        part4 = 4 * torch.stack([xp.sum((2, 4)), (xp * xp).sum((2, 4))], -1)
        assert_representable(part4, F32, 4 * k.vpb_r * cpg * 25)
        assert bool((k.sums == torch.stack([xp.sum((1, 2, 4)), (xp * xp).sum((1, 2, 4))], -1)).all())
        var = a.double() ** 2 * (m_ - m_ % 2) / m_
        rho = (a.double() / torch.sqrt(var + EPS)).reshape(n, groups)[:, torch.arange(c) // cpg]              # (n, C)
        assert float((rho - 1).abs().max()) < 1e-3
        g_, b_ = k.gamma.double(), k.beta.double()
        dy64, ref_b, ref_g, dmin, dmax = k.dy.double(), 0.0, 0.0, float("inf"), 0.0
        for sign in (1.0, -1.0, 0.0):
            z = sign * rho * g_ + b_                                     # (n, C): the value z takes where s == sign
            assert GN_Z_LO <= float(z.min()) and float(z.max()) <= GN_Z_HI, (float(z.min()), float(z.max()))
            d = _dsilu64(z)
            kk = (dy64 * (k.s == sign)).sum(1)                           # (n, C), integers
            ref_b = ref_b + (d * kk).sum(0)
            ref_g = ref_g + (sign * rho * d * kk).sum(0)
            dmin, dmax = min(dmin, float(d.abs().min())), max(dmax, float(d.abs().max()))
        assert dmin >= GN_D_MIN
        k.dbeta_ref, k.dgamma_ref = ref_b, ref_g
        for closed, auto in ((ref_b, k.dbeta), (ref_g, k.dgamma)):
            assert float((closed - auto).abs().max()) <= 1e-9 * max(1.0, float(auto.abs().max()))
        k.dparam_bound = GN_U * dy64.abs().sum((0, 1)) * dmax
        defect = dmin * min(1.0, float(rho.min()))                       # what one voxel with |dy| = 1 moves either sum by, at the least
        assert float(k.dparam_bound.max()) < 0.5 * defect, ("lower the density of dy", float(k.dparam_bound.max()), defect)
        assert int((k.dy != 0).sum()) > 0
    check_gn(k, cpu_gn(k), "cpu")
    return k


def cpu_gn(k, defect=None):
    """gn_stats / gn_silu_fwd / gn_silu_bwd_reduce / gn_silu_bwd_apply in fp32 torch on the CPU, rounded where the kernels round; with
    ``defect``: "stats-workgroup-missing" (one workgroup's voxels out of the sums), "dgamma-last-workgroup-skipped" (the ragged last one)."""
    n, s_, c, groups, cpg, dt = k.n, k.s_, k.c, k.groups, k.cpg, k.dtype
    x, m_ = k.x, float(k.s_ * k.cpg)
    sums = k.sums.clone()
    if defect == "stats-workgroup-missing":                              # workgroup 1 of sample 0
        lost = x[0, k.vpb_r:2 * k.vpb_r].double().reshape(-1, groups, cpg)
        sums[0] -= torch.stack([lost.sum((0, 2)), (lost * lost).sum((0, 2))], -1)
    mean = k.sums[..., 0] / m_
    var = (k.sums[..., 1] / m_ - mean * mean).clamp_min(0.0)
    ch = torch.arange(c) // cpg
    mu, rs = mean.float()[:, None, ch], torch.rsqrt(var.float() + EPS)[:, None, ch]                      # (n, 1, C)
    aa = rs * k.gamma
    bb = k.beta - mu * aa
    z = x * aa + bb
    sg = torch.sigmoid(z)
    y = _q(z * sg, dt)
    dz = k.dy * (sg * (1 + z * (1 - sg)))
    keep = torch.ones((n, s_, 1))
    if defect == "dgamma-last-workgroup-skipped":                        # the ragged last workgroup of the last sample
        keep[n - 1, (k.nblk - 1) * k.vpb_r:] = 0.0
    t1 = dz * (x - mu) * rs
    dgamma, dbeta = (t1 * keep).double().sum((0, 1)).float(), (dz * keep).double().sum((0, 1)).float()
    cs1, cs2 = t1.double().sum(1), dz.double().sum(1)                    # (n, C)
    m1 = ((k.gamma.double() * cs2).reshape(n, groups, cpg).sum(-1) / m_).float()[:, None, ch]
    m2 = ((k.gamma.double() * cs1).reshape(n, groups, cpg).sum(-1) / m_).float()[:, None, ch]
    k3 = rs * rs * m2
    dx = _q(aa * dz - (rs * m1 - k3 * mu) - x * k3, dt)
    return {"sums": sums, "y": y, "dx": dx, "dgamma": dgamma, "dbeta": dbeta}


def check_gn(k, res, route):
    """Every assertion of a case on {sums (n, G, 2) fp64; y, dx (n, S, C); dgamma, dbeta (C)}; a route may return a part of them."""
    what = f"{route} {k.family} {k.dtype} (shape {k.shape}, groups {k.groups})"
    _finite(res, what)
    f32 = k.dtype == F32
    if "sums" in res:
        if k.family == "B":
            _exact(res["sums"], k.sums, what, "sums")
        else:                                                            # fp32 partials of at most vpb x C/G terms, then fp64: 16 x 2^-24 of sum|term|
            _within(res["sums"], k.sums, 2.0 ** -20 * k.sums_abs, what, route, f"{k.family} sums")
    if "y" in res:                                                       # test_gpu_ops.py::test_group_norm_silu
        _bar(res["y"], k.y, 1e-3 if f32 else 2e-2, 1e-4 if f32 else 2e-2, what, route, f"{k.family} y")
    if "dx" in res:
        _bar_scaled(res["dx"], k.dx, 1e-3 if f32 else 3e-2, what, route, f"{k.family} dx")
    if "dgamma" in res:
        if k.family == "B":
            _within(res["dgamma"], k.dgamma_ref, k.dparam_bound, what, route, "B dgamma")
            _within(res["dbeta"], k.dbeta_ref, k.dparam_bound, what, route, "B dbeta")
        else:
            _bar_scaled(res["dgamma"], k.dgamma, 1e-3 if f32 else 3e-2, what, route, f"{k.family} dgamma")
            _bar_scaled(res["dbeta"], k.dbeta, 1e-3 if f32 else 3e-2, what, route, f"{k.family} dbeta")


# shape, groups, dtype, then what the shape is there for: voxels per reducing workgroup, reducing workgroups per sample, voxels per
# streaming workgroup
GN_SHAPES = [((2, 2, 192, 201, 16), 8, BF16, 151, 512, 128),    # two-row trip and single-row tail in one workgroup, ragged last workgroup,
             ((2, 2, 192, 201, 8), 8, F32, 151, 512, 128),      # finalize runs its unrolled loop 8 times
             ((4, 3, 256, 256, 16), 8, BF16, 768, 256, 192),    # the streaming passes leave the 128-voxel floor
             ((1, 3, 48, 60, 128), 8, BF16, 128, 68, 128),      # 16 voxel rows per pass, 4 two-row trips; finalize: one unrolled trip and a remainder
             ((1, 1, 17, 23, 12), 4, F32, 128, 4, 128),         # 3 channel vectors: the LDS-gather column_reduce, an idle thread, slabs of odd size
             ((1, 1, 17, 23, 24), 4, BF16, 128, 4, 128)]
GN_POOL = [((2, 2, 192, 200, 16), 8, BF16, 150, 512, 128), ((2, 2, 192, 200, 8), 8, F32, 150, 512, 128)]
GN_MEAN8 = GN_SHAPES[1]


def _gn_regime(k, vpb_r, nblk, vpb_s):
    assert (k.vpb_r, k.nblk, k.vpb_s) == (vpb_r, nblk, vpb_s), ((k.vpb_r, k.nblk, k.vpb_s), "the kernels' grid choice moved: re-derive the shapes")


def _gn_host_cases():
    cs = [(f"gn-{fam}-{sh}-{dt}", functools.partial(gn_case, fam, sh, g, dt)) for fam in ("G", "B") for sh, g, dt, *_ in GN_SHAPES + GN_POOL]
    return cs + [(f"gn-G8-{GN_MEAN8[0]}", functools.partial(gn_case, "G8", GN_MEAN8[0], GN_MEAN8[1], GN_MEAN8[2]))]


def _gn_defect_check(make, defect, first):
    k = make()
    if defect is None:
        check_gn(k, cpu_gn(k), "cpu")
        return
    with pytest.raises(AssertionError, match=rf"\): {first}: \d+/\d+ "):
        check_gn(k, cpu_gn(k, defect), "cpu")


def _gn_defect_checks():
    out = []
    for sh, g, dt in (((2, 2, 20, 21, 16), 8, BF16), ((1, 1, 17, 23, 12), 4, F32)):                    # 840 / 391 voxels: a ragged last workgroup
        mk = functools.partial(gn_case, "B", sh, g, dt)
        out.append((f"gn-B-{dt}-clean", functools.partial(_gn_defect_check, mk, None, None)))
        out.append((f"gn-B-{dt}-stats-workgroup-missing", functools.partial(_gn_defect_check, mk, "stats-workgroup-missing", "sums")))
        out.append((f"gn-B-{dt}-dgamma-last-workgroup-skipped", functools.partial(_gn_defect_check, mk, "dgamma-last-workgroup-skipped", "B dgamma")))
    return out


HOST_CHECKS = _ln_host_cases() + _gn_host_cases()
HOST_CHECKS += [(f"ln-routes-{fam}-{dt}", functools.partial(_ln_routes_on_cpu, functools.partial(ln_case, fam, 403, 64, dt)))
                for fam in ("G", "B") for dt in (BF16, F32)]
DEFECT_CHECKS = _ln_defect_checks() + [("ln-B-dscale-alone", _ln_dscale_alone_sees_a_row)] + _gn_defect_checks()


# =========================================================================================== GPU runners
def _ops():
    from video_vae_amd import ops
    return ops


def _poison(dev, nbytes):
    """Fill the allocator's free blocks of an output's size with NaN bit patterns: the ops allocate their own outputs, and a block that a
    route before this one left holding the right values would otherwise let an element no kernel wrote pass.  Best effort, no proof."""
    blocks = [torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev) for _ in range(6)]
    torch.cuda.synchronize()
    del blocks


def run_ln(k, dev, route):
    ops = _ops()
    dt, rows, c = k.dtype, k.rows, k.c
    _poison(dev, rows * c * (2 if dt == BF16 else 4))
    sc, bi = k.gamma.to(dev).requires_grad_(True), k.beta.to(dev).requires_grad_(True)
    dy, res = k.dy.to(dev, dt), {}
    if route == "strided":
        hd = k.heads * HEAD_DIM
        qkv = k.qkv.to(dev, dt).requires_grad_(True)
        view = qkv[:, hd:2 * hd].unflatten(-1, (k.heads, HEAD_DIM))      # the k third: rows strided in two levels, no gather copy
        assert not view.is_contiguous() and ops.layer_norm_supported(view)
        y = ops.layer_norm(view, sc, bi)
        y.backward(dy.reshape(y.shape))
        g = qkv.grad
        assert float(g[:, :hd].abs().max()) == 0.0 and float(g[:, 2 * hd:].abs().max()) == 0.0, "a gradient landed in the q or v third"
        dx = g[:, hd:2 * hd]
    elif route == "add":
        sk, oo = k.skip.to(dev, dt).requires_grad_(True), k.o.to(dev, dt).requires_grad_(True)
        y, xs = ops.add_layer_norm_fork(sk, oo, sc, bi)
        torch.autograd.backward([y, xs], [dy, k.dskip.to(dev, dt)])
        assert torch.equal(xs.detach().cpu().float(), k.x), "the sum the add route wrote is not round(skip + o)"
        assert torch.equal(sk.grad, oo.grad)
        dx = sk.grad
    else:
        x = k.x.to(dev, dt).requires_grad_(True)
        assert ops.layer_norm_supported(x)
        if route == "fork":
            y, skip = ops.layer_norm_fork(x, sc, bi)
            torch.autograd.backward([y, skip], [dy, k.dskip.to(dev, dt)])
        else:
            y = ops.layer_norm(x, sc, bi)
            y.backward(dy)
        dx = x.grad
    torch.cuda.synchronize()
    res.update(y=y.detach().reshape(rows, c).cpu(), dx=dx.reshape(rows, c).cpu(), dscale=sc.grad.cpu(), dbias=bi.grad.cpu())
    return res


def _ln_regime(k, edge=False):
    """The case sweeps: the backward grid is at its cap, the rows go past one sweep of it and end inside a sweep, and (contiguous rows,
    more than one row per wave-iteration) inside a wave-iteration.  ``edge``: the rows sit at the cap boundary instead."""
    ops = _ops()
    fwd, bwd, rpw = ln_sweeps(k.c, k.dtype)
    blocks = ops.lib().vvae_layernorm_bwd_blocks(k.rows, k.c, ops.DT[k.dtype])
    assert blocks == LN_BWD_CAP, (blocks, "the backward cap moved: re-derive the shapes")
    assert bwd == blocks * LN_BW * rpw
    if edge:
        assert abs(k.rows - bwd) <= 1
    else:
        assert k.rows > bwd and k.rows % bwd != 0 and k.rows % fwd != 0, (k.rows, fwd, bwd)
        assert k.heads or rpw == 1 or k.rows % rpw != 0, (k.rows, rpw)
    return fwd, bwd


def run_gn(k, dev, route):
    ops = _ops()
    dt = k.dtype
    _poison(dev, k.n * k.s_ * k.c * (2 if dt == BF16 else 4))
    x = k.x.reshape(k.shape).to(dev, dt)
    if route == "stats":
        res = {"sums": ops.gn_stats_raw(x, k.groups)}
    elif route == "pool":
        sc, bi = k.gamma.to(dev), k.beta.to(dev)
        assert ops.gn_silu_pool_ok(x, k.groups)
        y, pooled = ops.group_norm_silu(x, sc, bi, k.groups, EPS, pool=True)
        res = {"y": y.reshape(k.n, k.s_, k.c), "pooled": pooled}
    else:
        x.requires_grad_(True)
        sc, bi = k.gamma.to(dev).requires_grad_(True), k.beta.to(dev).requires_grad_(True)
        y = ops.group_norm_silu(x, sc, bi, k.groups, EPS)
        y.backward(k.dy.reshape(k.shape).to(dev, dt))
        res = {"y": y.detach().reshape(k.n, k.s_, k.c), "dx": x.grad.reshape(k.n, k.s_, k.c), "dgamma": sc.grad, "dbeta": bi.grad}
    torch.cuda.synchronize()
    return {name: t.cpu() for name, t in res.items()}


def _gn_regime_gpu(k):
    ops = _ops()
    floats = ops.lib().vvae_gn_part_floats(k.n, k.s_, k.c)
    assert floats == k.n * k.nblk * k.c * 2, (floats, k.n, k.nblk, k.c, "the reducing grid moved: re-derive the shapes")


# =========================================================================================== GPU tests
@pytest.mark.parametrize("family", ["G", "B"])
@pytest.mark.parametrize("dtype,c,rows", LN_SWEEPS)
def test_layer_norm_past_one_sweep(dev, dtype, c, rows, family):
    """ops.layer_norm, layer_norm_fork with a skip gradient and add_layer_norm_fork on one case and one fp64 reference."""
    k = ln_case(family, rows, c, dtype)
    fwd, _ = _ln_regime(k)
    assert rows > fwd, (rows, fwd)
    for route in LN_ROUTES:
        check_ln(k, run_ln(k, dev, route), route)
        _report(route)


@pytest.mark.parametrize("family", ["G", "B"])
@pytest.mark.parametrize("dtype,c,rows", LN_CAP_EDGE)
def test_layer_norm_at_the_backward_cap(dev, dtype, c, rows, family):
    k = ln_case(family, rows, c, dtype)
    _ln_regime(k, edge=True)
    check_ln(k, run_ln(k, dev, "plain"), "plain")
    _report("plain")


def test_layer_norm_mean_8(dev):
    dtype, c, rows = LN_MEAN8
    k = ln_case("G8", rows, c, dtype)
    _ln_regime(k)
    check_ln(k, run_ln(k, dev, "plain"), "plain")
    _report("plain")


@pytest.mark.parametrize("family", ["G", "B"])
@pytest.mark.parametrize("dtype,heads,tokens", LN_STRIDED)
def test_layer_norm_strided_head_view_past_one_sweep(dev, dtype, heads, tokens, family):
    """The k third of a fused (tokens, 3 heads 64) buffer, forward and backward: both kernels read x through row_off."""
    k = ln_case(family, tokens * heads, HEAD_DIM, dtype, heads)
    fwd, _ = _ln_regime(k)
    assert k.rows > fwd or (dtype, tokens) == (F32, 4100), (k.rows, fwd)
    check_ln(k, run_ln(k, dev, "strided"), "strided")
    _report("strided")


@pytest.mark.parametrize("family", ["G", "B"])
@pytest.mark.parametrize("shape,groups,dtype,vpb_r,nblk,vpb_s", GN_SHAPES)
def test_group_norm_silu_past_the_floor(dev, shape, groups, dtype, vpb_r, nblk, vpb_s, family):
    """gn_stats_raw, then group_norm_silu forward and backward."""
    k = gn_case(family, shape, groups, dtype)
    _gn_regime(k, vpb_r, nblk, vpb_s)
    _gn_regime_gpu(k)
    check_gn(k, run_gn(k, dev, "stats"), "gn-stats")
    check_gn(k, run_gn(k, dev, "fwd-bwd"), "gn")
    _report("gn-stats")
    _report("gn")


def test_group_norm_silu_mean_8(dev):
    shape, groups, dtype, vpb_r, nblk, vpb_s = GN_MEAN8
    k = gn_case("G8", shape, groups, dtype)
    _gn_regime(k, vpb_r, nblk, vpb_s)
    _gn_regime_gpu(k)
    check_gn(k, run_gn(k, dev, "stats"), "gn-stats")
    check_gn(k, run_gn(k, dev, "fwd-bwd"), "gn")
    _report("gn-stats")
    _report("gn")


@pytest.mark.parametrize("family", ["G", "B"])
@pytest.mark.parametrize("shape,groups,dtype,vpb_r,nblk,vpb_s", GN_POOL)
def test_group_norm_silu_with_pool_past_the_floor(dev, shape, groups, dtype, vpb_r, nblk, vpb_s, family):
    """gn_stats_raw at the even width, then group_norm_silu(pool=True): y against fp64, the pooled output bitwise the (1, 2, 2) max-pool
    of the y it stored."""
    k = gn_case(family, shape, groups, dtype)
    _gn_regime(k, vpb_r, nblk, vpb_s)
    _gn_regime_gpu(k)
    check_gn(k, run_gn(k, dev, "stats"), "gn-stats")
    res = run_gn(k, dev, "pool")
    pooled = res.pop("pooled")
    check_gn(k, res, "gn-pool")
    want = O.max_pool_1x2x2(res["y"].reshape(shape).float())
    assert tuple(pooled.shape) == tuple(want.shape)
    assert_exact(pooled.float(), want.double(), "gn-pool: pooled against max_pool_1x2x2 of the stored y")
    _report("gn-stats")
    _report("gn-pool")
