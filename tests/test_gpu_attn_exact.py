"""Exact softmax families for the attention kernels, forward and backward: every key counts exactly once, or exactly one key counts.

Attention has a softmax in it, so integer inputs alone do not make it exact.  Two input families do, through arguments the op takes anyway
(q_scale, k_scale, the RoPE tables):

  * Family U, uniform softmax.  q_scale = 0: q is exactly 0 behind the norm, every score is 0 and P = 1/L over the L attended keys.  k is
    Gaussian, k_scale and the RoPE tables are the real ones (those code paths stay live), v and dO are small integers.  Then
    out = sum(v_j, j < L) / L for EVERY query, dv_j = sum_i(dO_i) / L for j < L and exactly 0 for a masked j, the dq and dk sections and
    dk_scale are exactly 0, lse = ln L.  dq_scale alone is non-trivial and goes against the oracle's autograd at the existing 5e-2 of scale.
    A dropped or doubled key moves a value by 1/L of a key's v: with L a power of two every expected value is a bf16 number and the
    comparison is at zero tolerance; for any other L the probability and the output are each rounded once to bf16 (2^-8 relative at the
    most each), so |got - want| <= 2^-7 |want| with got exactly 0 where want is 0 -- and because the builder asserts |sum v| <= 63 and
    |sum dO| <= 63 before any GPU result is looked at, 1/L is always more than that bound allows.  fp32: rtol 1e-5, atol 1e-6.

  * Family H, one-hot softmax.  Keys and queries are rows of the Sylvester Hadamard matrix (+-1, every aligned block of 4 columns sums
    to 0, two different codes have dot 0 or -D), pre-rotated by the inverse of their own position through quarter-turn RoPE tables (cos,
    sin in {0, +-1}: a signed permutation, exact in any arithmetic).  The norm returns exactly +-scale in bf16, the matched logit beats
    every other by scale^2 sqrt(D) >= 128 nats, every other probability underflows to 0.  out_i = mean of v over the attended keys that
    carry query i's code (1, 2 or 4 of them: ties walk equal maxima across key tiles), dv_j = sum of dO_i / copies over the queries that
    select j, lse = matched logit + ln(copies).  With one key per code dS = P (dP - delta) is exactly 0, and so are dq, dk, dq_scale and
    dk_scale.  With 2 or 4 keys per code dS is not 0 (the v of a tie group differ): the gradients behind it are 0 only up to the norm's
    eps and to cancellation over the tie group, and are held to the bounds derived in _tie_bounds.  A masked tail carries decoys -- the
    code of an attended key with a different v -- so a kernel that misreads the mask ties with the decoy.  bf16: out and dv at zero
    tolerance throughout; fp32 at Family U's bar (the prep pass keeps the norm's 1 / sqrt(1 + eps) there, see check_prep).

The builders validate every case on the CPU (the oracle, in the case's dtype, passes the same assertions) before a GPU result is looked
at; tests/test_host.py runs them without a GPU (HOST_CHECKS) and feeds the assertions CPU results with one defect each (DEFECT_CHECKS):
every one of them must raise.

Routes: the fused spatial kernels (attn_spatial.hip), the prep kernels around the library core (qk_prep.hip), the generic temporal
kernels (attn_temporal.hip), the VALU lane-per-frame kernels at every lanes-per-row setting (attn_temporal_fast.hip), the matrix-core
kernels at T = 16 (attn_temporal_mfma.hip, grid capped and not) and at T = 32 / 64 (attn_temporal_mfma32.hip).  Each test asserts the
route it means to exercise.
"""
import functools
import math
import types
import zlib

import pytest
import torch

from oracle import layers as OL
from oracle import nn as O
from util import assert_abs, assert_close, assert_close_scaled, assert_exact, assert_rounded, ints, rnd

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
F32_RTOL, F32_ATOL = 1e-5, 1e-6          # fp32 outputs: about 40 ulp for exp / rcp / log intrinsics good to a few ulp; the smallest defect is 1/64
# Family H in fp32 uses most of these two bars with tie groups: P = exp(s - lse) with s and lse near 128 .. 362, where fp32 is spaced
# 1.5e-5 .. 3e-5, so P = 1/2 carries about one such spacing (the VALU kernels reach 0.95 of the dv bar and 9.7e-5 of the lse bar).  A
# failure just above either bar after a reordering of that arithmetic is this effect, not a dropped key (which moves a value by 1/4).
BF16_REL = 2.0 ** -7                     # bf16, L no power of two: P rounded once, the output rounded once, 2^-8 relative each at the most
LSE_ATOL_U, LSE_ATOL_H = 1e-5, 1e-4      # ln L <= 5.6; the one-hot logits sit near 185 .. 362, where fp32 is spaced 1.5e-5 .. 3e-5
FIGURES = {}                             # (route, what) -> largest error seen against the fp64 reference (printed by the GPU tests)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31 - 1000)


def _randint(hi, n, gen):
    return torch.randint(0, hi, (n,), generator=gen)


def _mask_lens(kind, a, t, mask_div):
    """Attended lengths, one per mask row: every row a different tail (None: no mask)."""
    if kind == "none":
        return None
    nm = (a + mask_div - 1) // mask_div
    return torch.tensor([max(1, t - (i * 5 + 3) % t) for i in range(nm)])


def _common(family, a, t, heads, d, dtype, mask, mask_div, inner, maxlen):
    c = types.SimpleNamespace(family=family, a=a, t=t, heads=heads, d=d, hd=heads * d, dtype=dtype, mask=mask, inner=inner, maxlen=maxlen)
    c.mask_div = mask_div if mask == "shared" else 1                     # "rows": one mask row per sequence, whatever the layout
    c.lens_rows = _mask_lens(mask, a, t, c.mask_div)
    c.lens = torch.full((a,), t) if c.lens_rows is None else c.lens_rows[torch.arange(a) // c.mask_div]
    c.att = torch.arange(t)[None, :] < c.lens[:, None]                                   # (a, t) bool: key j of sequence a is attended
    c.mask_u8 = None if c.lens_rows is None else (torch.arange(t)[None, :] < c.lens_rows[:, None]).to(torch.uint8)
    return c


# =========================================================================================== Family U
@functools.lru_cache(maxsize=None)
def uniform_case(a, t, heads, d, dtype, mask="none", mask_div=1, inner=1, maxlen=64, density=0.5):
    c = _common("U", a, t, heads, d, dtype, mask, mask_div, inner, maxlen)
    seed = _seed("U", a, t, heads, d, mask, mask_div, inner)
    hd = c.hd
    v = ints((a, t, hd), seed + 2, -1, 1, density)
    c.go = ints((a, t, hd), seed + 3, -1, 1)
    c.qkv = torch.cat([rnd((a, t, hd), seed), rnd((a, t, hd), seed + 1), v], -1).to(dtype).float()
    c.qs = torch.zeros(d)
    c.ks = 1 + 0.2 * rnd((d,), seed + 4)
    cos, sin = OL.rope_tables(d, maxlen)
    c.cos, c.sin = O.q(cos, dtype), O.q(sin, dtype)                      # as the kernels take them: rounded once to the activation dtype
    att = c.att[:, :, None, None].double()
    sv = (v.double().reshape(a, t, heads, d) * att).sum(1)               # (a, heads, d)
    sg = c.go.double().reshape(a, t, heads, d).sum(1)                    # every query, the ones at or beyond L included
    assert float(sv.abs().max()) <= 63 and float(sg.abs().max()) <= 63, ("lower the density", float(sv.abs().max()), float(sg.abs().max()))
    L = c.lens.double()[:, None, None]
    c.out = (sv / L)[:, None].expand(a, t, heads, d).contiguous()
    c.dv = (sg / L)[:, None] * att
    c.lse = torch.log(L).expand(a, heads, t).reshape(a * heads, t)
    c.lse_atol = LSE_ATOL_U
    pow2 = (c.lens & (c.lens - 1)) == 0
    c.rel = torch.where(pow2, 0.0, BF16_REL).double()[:, None, None, None]
    c.all_exact = bool(pow2.all())
    c.zero_tol = {"dq": 0.0, "dk": 0.0, "dk_scale": 0.0}                 # q is exactly 0 behind the norm: 0 x finite, in any arithmetic
    if c.all_exact and dtype == BF16:
        assert bool((c.out.to(BF16).double() == c.out).all()) and bool((c.dv.to(BF16).double() == c.dv).all())
    ref = oracle_result(c)                                               # dq_scale is the one non-trivial gradient left: oracle autograd
    c.dq_scale = ref["dq_scale"]
    assert float(c.dq_scale.abs().max()) > 0
    check(c, ref, "oracle")
    return c


# =========================================================================================== Family H
def hadamard_codes(d):
    """Rows r of the Sylvester Hadamard matrix of order d with r & 3 != 0, and their negatives: (1.5 d, d) of +-1."""
    r = torch.arange(d)
    bits = r[:, None] & r[None, :]
    par = torch.zeros_like(bits)
    for b in range(d.bit_length()):
        par ^= (bits >> b) & 1
    h = (1 - 2 * par).float()
    rows = h[(r & 3) != 0]
    codes = torch.cat([rows, -rows], 0)
    assert bool((codes.reshape(codes.shape[0], d // 4, 4).sum(-1) == 0).all())
    g = codes @ codes.T
    off = g[~torch.eye(codes.shape[0], dtype=torch.bool)]
    assert bool(((off == 0) | (off == -d)).all()) and bool((g.diagonal() == d).all())
    return codes


def quarter_turn_tables(d, maxlen, seed):
    """RoPE tables with angle (pi / 2) g(p, j // 4), g a seeded integer in 0..3 per position and block of 4 frequency indices; the two
    halves identical as in the real tables.  cos, sin in {0, +-1}."""
    h = d // 2
    g = torch.randint(0, 4, (maxlen, max(1, h // 4)), generator=torch.Generator().manual_seed(seed))
    gj = g[:, torch.arange(h) // 4]
    cq, sq = torch.tensor([1.0, 0.0, -1.0, 0.0]), torch.tensor([0.0, 1.0, 0.0, -1.0])
    return torch.cat([cq[gj], cq[gj]], -1), torch.cat([sq[gj], sq[gj]], -1)


def _group_sizes(n, copies):
    """n keys in groups of `copies`, the rest in smaller powers of two: every group size is a power of two."""
    out, c = [], copies
    while n:
        while c > n:
            c //= 2
        out.append(c)
        n -= c
    return out


def _tie_bounds(c, ds):
    """What "zero" means for dq, dk and the scale gradients of a one-hot case.  With one key per code dS = P (dP - delta) is exactly 0
    (dP and delta are the same integer dot product) and so is everything behind it: zero tolerance.  With 2 or 4 keys per code dS is
    not 0: dS_ij = (dP_ij - mean over the tie group) / copies.  The key gradient behind the rotation is then b_j x_j, a multiple
    b_j = sum_i(dS_ij) scale / sqrt(D) of the key's own normalised row x_j, and the norm backward removes that direction up to its eps:
    dk_j = b_j scale (1 - 1 / (1 + eps)) x_j / sqrt(1 + eps), about b_j scale eps.  It is computed as a difference of two terms of size
    b_j scale, each good to a few fp32 ulp (2^-24 << eps), so |dk| <= 2 eps scale max|b|.  Over a tie group the dS_ij of a query sum to 0,
    so dq behind the rotation, dq_scale and dk_scale are 0 in exact arithmetic, as sums of terms dS_ij scale / sqrt(D) that cancel.  In
    fp32 every term carries a few roundings (a factor 1 / sqrt(D) that is no power of two, an approximate reciprocal in P) and is
    allowed 2^-20 of its size, 16 times what two roundings take.  In bf16 the gradient behind the rotation may be held in bf16 before
    the norm backward (the library core returns it so, the oracle's emulation rounds it too): one rounding to nearest, 2^-9 of the
    rounded number at the most.  For dk_scale the rounded numbers are the b_j (the sum over the queries is taken in fp32 first), for
    dq_scale the single terms.  These are worst-case sums over every token and head, which is what a scale gradient sums over; the
    errors of a correct kernel add like a random walk and use a few percent of them (the GPU tests print the fraction used).
    dq gets dk's bound: its rows are multiples of the query's own row as well."""
    if float(ds.abs().max()) == 0.0:
        return {"dq": 0.0, "dk": 0.0, "dq_scale": 0.0, "dk_scale": 0.0}
    f = c.scale / math.sqrt(c.d)
    row = 2 * EPS * c.scale * f * float(ds.sum(2).abs().max()) * (1 + BF16_REL)
    u = 2.0 ** -9 if c.dtype == BF16 else 2.0 ** -20
    return {"dq": row, "dk": row, "dq_scale": u * f * float(ds.abs().sum()), "dk_scale": u * f * float(ds.sum(2).abs().sum())}


@functools.lru_cache(maxsize=None)
def onehot_case(a, t, heads, d, dtype, copies=1, mask="none", mask_div=1, inner=1, maxlen=64, scale=None):
    c = _common("H", a, t, heads, d, dtype, mask, mask_div, inner, maxlen)
    seed = _seed("H", a, t, heads, d, copies, mask, mask_div, inner)
    gen = torch.Generator().manual_seed(seed)
    hd = c.hd
    codes = hadamard_codes(d)
    c.copies = copies
    c.scale = float(scale if scale is not None else (4 if d == 64 else 8))
    c.qs = torch.full((d,), c.scale)
    c.ks = torch.full((d,), c.scale)
    c.cos, c.sin = quarter_turn_tables(d, maxlen, seed + 1)
    v = ints((a, t, hd), seed + 2, -2, 2).reshape(a, t, heads, d)
    c.go = ints((a, t, hd), seed + 3, -2, 2)
    kcode = torch.zeros((a, t, heads), dtype=torch.long)
    qcode = torch.zeros((a, t, heads), dtype=torch.long)
    c.decoys = []                                                        # (sequence, key): masked keys that carry an attended key's code
    for s in range(a):
        L = int(c.lens[s])
        for h in range(heads):
            sizes = _group_sizes(L, copies)
            assert len(sizes) <= codes.shape[0], (len(sizes), codes.shape[0])
            pick = torch.randperm(codes.shape[0], generator=gen)[:len(sizes)]
            ks_ = torch.repeat_interleave(pick, torch.tensor(sizes))[torch.randperm(L, generator=gen)]
            kcode[s, :L, h] = ks_
            for j in range(L, t):                                        # the masked tail: decoys, same code as an attended key, another v
                src = int(_randint(L, 1, gen))
                kcode[s, j, h] = kcode[s, src, h]
                if bool((v[s, j, h] == v[s, src, h]).all()):
                    v[s, j, h, 0] = v[s, src, h, 0] + 1 if v[s, src, h, 0] < 2 else -2
                if h == 0:
                    c.decoys.append((s, j))
            tgt = torch.randperm(L, generator=gen).repeat((t + L - 1) // L)[:t][torch.randperm(t, generator=gen)]
            qcode[s, :, h] = kcode[s, tgt, h]                            # every query, the masked frames' too, targets an attended key
    c.qcode, c.kcode = qcode, kcode
    wq, wk = codes[qcode], codes[kcode]                                  # (a, t, heads, d): what q and k must be BEHIND the rotation
    qi, ki = OL.rope(wq, wk, c.cos, -c.sin)                              # each token rotated back by its own position
    assert bool((qi.abs() == 1).all()) and bool((ki.abs() == 1).all())
    assert bool((qi.sum(-1) == 0).all()) and bool((ki.sum(-1) == 0).all())               # mean 0, variance 1: the norm returns +-scale
    c.qkv = torch.cat([qi.reshape(a, t, hd), ki.reshape(a, t, hd), v.reshape(a, t, hd)], -1)
    c.prep = c.scale * torch.cat([wq.reshape(a, t, hd), wk.reshape(a, t, hd)], -1).double()
    m = (qcode.permute(0, 2, 1)[:, :, :, None] == kcode.permute(0, 2, 1)[:, :, None, :]) & c.att[:, None, None, :]      # (a, heads, i, j)
    cnt = m.sum(-1)
    assert bool((cnt > 0).all()) and bool(((cnt & (cnt - 1)) == 0).all()) and int(cnt.max()) <= max(copies, 1)
    p = m.double() / cnt[..., None].double()
    v64, g64 = v.double(), c.go.double().reshape(a, t, heads, d)
    c.out = torch.einsum("ahij,ajhd->aihd", p, v64)
    c.dv = torch.einsum("ahij,aihd->ajhd", p, g64)
    # dS = P (dP - delta) is no sum: it has to be a number of the dtype for the tie groups to cancel exactly in dq and dk_scale
    ds = p * (torch.einsum("aihd,ajhd->ahij", g64, v64) - torch.einsum("aihd,aihd->ahi", g64, c.out)[..., None])
    for name, x in (("out", c.out), ("dv", c.dv), ("dS", ds)):
        assert bool((x.to(BF16).double() == x).all()), f"{name} is no bf16 number: another seed or fewer copies"
    logit = c.scale ** 2 * math.sqrt(d) / (1.0 if dtype == BF16 else 1.0 + EPS)          # fp32 keeps the norm's 1 / sqrt(1 + eps)
    assert logit > 110                                                   # every other probability is below e^-110 < 2^-149: exactly 0
    c.lse = (logit + torch.log(cnt.double())).reshape(a * heads, t)
    c.lse_atol = LSE_ATOL_H
    c.rel = torch.zeros((1, 1, 1, 1), dtype=torch.float64)
    c.all_exact = True
    c.dq_scale = torch.zeros(d, dtype=torch.float64)
    c.zero_tol = _tie_bounds(c, ds)
    check(c, oracle_result(c), "oracle")                                 # the oracle, in the case's dtype, returns exactly these bits
    return c


# =========================================================================================== the oracle, and the oracle with one defect
DEFECTS = ("drop-key", "double-key", "mask-off-by-one", "tables-shifted", "blocks-swapped", "decoy-unmasked", "dv-query-dropped")


def oracle_result(c, defect=None):
    """The CPU oracle on the case's inputs in the case's dtype -> {out, dqkv, dq_scale, dk_scale, lse}; with ``defect`` it makes one
    of the mistakes tiled attention kernels make."""
    a, t, heads, d, hd, dtype = c.a, c.t, c.heads, c.d, c.hd, c.dtype
    x = c.qkv.clone().requires_grad_(True)
    qs, ks = c.qs.clone().requires_grad_(True), c.ks.clone().requires_grad_(True)
    q, k, v = (z.reshape(a, t, heads, d) for z in torch.chunk(x, 3, dim=-1))
    cos, sin = c.cos, c.sin
    if defect == "tables-shifted":
        cos, sin = cos[1:], sin[1:]
    if defect == "blocks-swapped":                                       # frequency blocks 0 and 1 (4 indices each) trade places, in both halves
        idx = torch.arange(d)
        j = idx % (d // 2)
        idx = torch.where(j < 4, idx + 4, torch.where(j < 8, idx - 4, idx))
        cos, sin = cos[:, idx], sin[:, idx]
    qr, kr = OL.rope(O.layer_norm(q, qs, None, dtype), O.layer_norm(k, ks, None, dtype), cos, sin, dtype)
    att = c.att.clone()
    if defect == "drop-key":                                             # the key query 0 of sequence 0 looks at (U: any attended key)
        j0 = 0 if c.family == "U" else int((c.kcode[0, :, 0] == c.qcode[0, 0, 0]).nonzero()[0])
        att[0, j0] = False
    if defect == "mask-off-by-one":                                      # one shared mask row one frame too long
        r = int((c.lens_rows < t).nonzero()[0])
        att[r * c.mask_div:(r + 1) * c.mask_div, int(c.lens_rows[r])] = True
    if defect == "decoy-unmasked":
        s, j = c.decoys[-1]
        att[s, j] = True
    if defect == "double-key":                                           # key 1 once more behind the last one
        kr, v, att = torch.cat([kr, kr[:, 1:2]], 1), torch.cat([v, v[:, 1:2]], 1), torch.cat([att, att[:, 1:2]], 1)
    mask = None if bool(att.all()) else att.reshape(a, 1, 1, -1)
    out = OL.dot_product_attention(qr, kr, v, mask, dtype).reshape(a, t, hd)
    go = c.go.clone()
    out.backward(go, retain_graph=defect == "dv-query-dropped")
    dqkv = x.grad.clone()
    if defect == "dv-query-dropped":                                     # query 3 of sequence 0 missing from dV
        go[0, 3] = 0
        x.grad = None
        out.backward(go)
        dqkv[..., 2 * hd:] = x.grad[..., 2 * hd:]
    with torch.no_grad():
        sc = torch.einsum("aihd,ajhd->ahij", qr.double(), kr.double()) / math.sqrt(d)
        sc = sc.masked_fill(~att[:, None, None, :], -float("inf"))
        lse = torch.logsumexp(sc, -1).reshape(a * heads, t)
    return {"out": out.detach(), "dqkv": dqkv, "dq_scale": qs.grad.clone(), "dk_scale": ks.grad.clone(), "lse": lse}


# =========================================================================================== the assertions
def _note(route, what, value):
    FIGURES[(route, what)] = max(FIGURES.get((route, what), 0.0), float(value))


def check(c, res, route):
    """Every assertion of a case on a result {out (a, t, heads d), dqkv (a, t, 3 heads d), dq_scale, dk_scale[, lse | lse2]}."""
    a, t, heads, d, hd = c.a, c.t, c.heads, c.d, c.hd
    sh = (a, t, heads, d)
    out = res["out"].reshape(sh)
    dq, dk, dv = (res["dqkv"][..., i * hd:(i + 1) * hd].reshape(sh) for i in range(3))
    tag = f"{route} {c.family} {c.dtype} (a {a}, t {t}, heads {heads}, d {d}, mask {c.mask}, inner {c.inner})"
    zero = torch.zeros(sh, dtype=torch.float64)
    for name, x in res.items():                                          # an element no kernel wrote (the buffers start as NaN) fails here
        assert bool(torch.isfinite(x.float()).all()), f"{tag}: {name} has {int((~torch.isfinite(x.float())).sum())} non-finite elements"
    if c.dtype == BF16:
        for name, got, want in (("out", out, c.out), ("dv", dv, c.dv)):
            if c.all_exact:
                assert_exact(got, want, f"{tag}: {name}")
            else:
                _note(route, f"{c.family} bf16 {name}, L no power of two: rel", assert_rounded(got, want, c.rel, f"{tag}: {name}"))
    else:
        for name, got, want in (("out", out, c.out), ("dv", dv, c.dv)):
            assert_close(got, want, rtol=F32_RTOL, atol=F32_ATOL, what=f"{tag}: {name}")
            err = (got.detach().double().cpu() - want).abs()
            _note(route, f"{c.family} fp32 {name}: abs", err.max())
            _note(route, f"{c.family} fp32 {name}: abs / bound", (err / (F32_ATOL + F32_RTOL * want.abs())).max())
        dead = ~c.att[:, :, None, None].expand(sh)
        assert_exact(dv.detach().cpu()[dead], zero[dead], f"{tag}: dv of the masked keys")
    zeros = [("dq", dq), ("dk", dk), ("dk_scale", res["dk_scale"])] + ([("dq_scale", res["dq_scale"])] if c.family == "H" else [])
    for name, got in zeros:
        if c.zero_tol[name] == 0.0:
            assert_exact(got, torch.zeros(got.shape, dtype=torch.float64), f"{tag}: {name}")
        else:
            assert_close(got, torch.zeros(got.shape), rtol=0.0, atol=c.zero_tol[name], what=f"{tag}: {name} (tie groups)")
            _note(route, f"H {name}, tie groups: abs / bound", float(got.detach().double().abs().max()) / c.zero_tol[name])
    if c.family == "U":
        assert_close_scaled(res["dq_scale"], c.dq_scale, rel=5e-2, what=f"{tag}: dq_scale")
    if "lse" in res:
        _note(route, f"{c.family} lse: abs", assert_abs(res["lse"], c.lse, c.lse_atol, f"{tag}: lse"))
    if "lse2" in res:
        _note(route, f"{c.family} lse2: abs", assert_abs(res["lse2"], c.lse / math.log(2.0), c.lse_atol, f"{tag}: lse2"))


# =========================================================================================== the cases, by route
def _case(family, a, t, heads, d, dtype, mask="none", mask_div=1, inner=1, maxlen=64, copies=None):
    if family == "U":
        return uniform_case(a, t, heads, d, dtype, mask, mask_div, inner, maxlen)
    if copies is None:                                                   # as few keys per code as the code count allows
        copies = 1
        while t > copies * (3 * d // 2):
            copies *= 2
    return onehot_case(a, t, heads, d, dtype, copies, mask, mask_div, inner, maxlen)


SPATIAL_U = [(2, 32, 3), (3, 64, 2), (2, 96, 2), (1, 160, 3), (2, 256, 2)]                 # (a, s, heads), head_dim 64, bf16
SPATIAL_H = [(2, 32, 3, 1), (1, 96, 2, 1), (1, 160, 2, 2), (2, 256, 2, 4)]                 # ... and keys per code
LIBRARY_H = [(2, 96, 4, 32, 4), (2, 48, 3, 16, 4), (1, 48, 2, 8, 4)]                       # (a, s, heads, d, keys per code)
GENERIC = [(4, 7, 2, 16), (5, 5, 4, 32), (3, 20, 3, 64), (2, 40, 2, 32), (3, 12, 2, 24)]   # head_dim 24: no Hadamard order, Family U only
# VALU lane-per-frame: (a, t, heads, d, inner, mask kind, mask_div).  head_dim 64 at T = 16 / 32 / 40 takes 4 / 2 / 1 lanes per row.
VALU = [(3, 16, 3, 64, 1, "none", 1), (3, 32, 2, 64, 1, "rows", 1), (3, 40, 2, 64, 1, "shared", 2),
        (5, 16, 2, 32, 1, "rows", 1), (3, 24, 3, 32, 1, "none", 1), (5, 16, 3, 16, 1, "shared", 2), (4, 24, 2, 16, 1, "rows", 1),
        (7, 16, 2, 8, 1, "none", 1), (3, 24, 3, 8, 1, "shared", 3),
        (8, 16, 2, 32, 4, "shared", 4), (8, 24, 2, 64, 4, "none", 1)]
MFMA16 = [(5, 3, 1), (12, 8, 4)]                                                           # (a, heads, inner): tests/test_gpu_tattn_persistent.py
MFMA32 = [(3, 32, 2), (2, 64, 3)]                                                          # (a, t, heads)
MASKS = ["none", "rows", "shared"]


def _shared_div(a, inner):
    return inner if inner > 1 else 2


def _all_cases():
    cs = []
    for fam in ("U", "H"):
        cs += [(f"spatial-{fam}-{c}", functools.partial(_case, fam, c[0], c[1], c[2], 64, BF16, maxlen=256, copies=(c[3] if fam == "H" else None)))
               for c in (SPATIAL_U if fam == "U" else SPATIAL_H)]
        for dt in (F32, BF16):
            for m in ("none", "rows"):
                cs += [(f"generic-{fam}-{dt}-{m}-{c}", functools.partial(_case, fam, *c, dt, m)) for c in GENERIC if fam == "U" or c[3] != 24]
            cs += [(f"valu-{fam}-{dt}-{c}", functools.partial(_case, fam, *c[:4], dt, c[5], c[6], c[4])) for c in VALU]
        for m in MASKS:
            cs += [(f"mfma16-{fam}-{m}-{c}", functools.partial(_case, fam, c[0], 16, c[1], 64, BF16, m, _shared_div(c[0], c[2]), c[2])) for c in MFMA16]
            cs += [(f"mfma32-{fam}-{m}-{c}", functools.partial(_case, fam, c[0], c[1], c[2], 64, BF16, m, 2)) for c in MFMA32]
    cs += [(f"library-H-{c}", functools.partial(_case, "H", *c[:4], BF16, maxlen=256, copies=c[4])) for c in LIBRARY_H]
    cs += [(f"prep-H-fp32-{c}", functools.partial(_case, "H", *c[:4], F32, maxlen=256, copies=c[4])) for c in LIBRARY_H]
    return cs


HOST_CHECKS = _all_cases()            # every builder validates its case against the oracle: tests/test_host.py runs them without a GPU


def _defect_checks():
    """One case of each family and dtype (T = 16, head_dim 64, a mask row shared by two sequences), the oracle's result with one defect
    -> the assertions must raise.  The table defects go to Family H alone: Family U's outputs do not depend on the tables by
    construction (q is 0), and its dq_scale sees only differences of positions, which a shift leaves alone."""
    out = []
    for fam in ("U", "H"):
        for dt in (BF16, F32):
            mk = functools.partial(_case, fam, 4, 16, 2, 64, dt, "shared", 2)
            for defect in (None,) + DEFECTS:
                if fam == "U" and defect in ("tables-shifted", "blocks-swapped", "decoy-unmasked"):
                    continue
                out.append((f"{fam}-{dt}-{defect or 'clean'}", functools.partial(_defect_check, mk, defect)))
    return out


def _defect_check(make, defect):
    """The assertion that has to fire is named, so another one raising by accident does not count.  A doubled key in Family H is
    seen by the lse assertion alone: the copy carries the same v, so out keeps its mean and dv its sum.  On the routes that return
    no lse (generic temporal, library core) a doubled key is therefore caught by Family U only, whose out and dv move by 1/L."""
    c = make()
    if defect is None:
        check(c, oracle_result(c), "oracle")
        return
    first = "dv" if defect == "dv-query-dropped" else "lse" if (c.family, defect) == ("H", "double-key") else "out"
    with pytest.raises(AssertionError, match=rf"\): {first}: \d+/\d+ "):
        check(c, oracle_result(c, defect), "oracle")


DEFECT_CHECKS = _defect_checks()


# =========================================================================================== GPU runners
def _ops():
    from video_vae_amd import ops
    return ops


def _p(x):
    return None if x is None else x.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _to_dev(x, c, dev):
    """(a, t, C) sequences -> the layout the kernels read: as they are, or (b, t, inner, C) with sequence b * inner + i strided over frames."""
    if c.inner > 1:
        x = x.reshape(c.a // c.inner, c.inner, c.t, -1).permute(0, 2, 1, 3)
    return x.contiguous().to(dev, c.dtype)


def _from_dev(y, c):
    y = y.reshape(c.a // c.inner, c.t, c.inner, -1).permute(0, 2, 1, 3) if c.inner > 1 else y
    return y.reshape(c.a, c.t, -1)


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)      # an element no kernel wrote can not pass for an exact 0


def _tables(c, dev):
    return c.cos.to(dev).contiguous(), c.sin.to(dev).contiguous()


def run_temporal_fast(c, dev):
    """vvae_temporal_attn_fwd_fast / _bwd_fast, whichever kernels they dispatch to."""
    ops = _ops()
    L = ops.lib()
    a, t, heads, d, hd, dt = c.a, c.t, c.heads, c.d, c.hd, ops.DT[c.dtype]
    qkv, go = _to_dev(c.qkv, c, dev).reshape(a * t, 3 * hd), _to_dev(c.go, c, dev).reshape(a * t, hd)
    qs, ks = c.qs.to(dev), c.ks.to(dev)
    cos, sin = _tables(c, dev)
    mask = None if c.mask_u8 is None else c.mask_u8.to(dev)
    assert mask is None or mask.data_ptr() % 4 == 0                      # a mask off a 4-byte boundary sends the dispatch to the VALU kernels
    nblk = L.vvae_temporal_attn_fast_blocks(a, t, heads, d, dt)
    out, lse = _nan((a * t, hd), c.dtype, dev), _nan((a * heads, t), F32, dev)
    dqkv, part = _nan((a * t, 3 * hd), c.dtype, dev), _nan((nblk, 2 * d), F32, dev)
    ops.check(L.vvae_temporal_attn_fwd_fast(_p(qkv), 3 * hd, _p(out), hd, _p(lse), _p(qs), _p(ks), _p(cos), _p(sin), _p(mask), c.mask_div,
                                            c.inner, a, t, heads, d, EPS, dt, _stream()), "fwd")
    ops.check(L.vvae_temporal_attn_bwd_fast(_p(qkv), 3 * hd, _p(out), hd, _p(go), hd, _p(lse), _p(dqkv), 3 * hd, _p(qs), _p(ks), _p(cos),
                                            _p(sin), _p(mask), c.mask_div, c.inner, _p(part), a, t, heads, d, EPS, dt, _stream()), "bwd")
    dqs, dks = ops.fold_partials(part, None, None, d)
    torch.cuda.synchronize()
    return {"out": _from_dev(out, c), "dqkv": _from_dev(dqkv, c), "dq_scale": dqs, "dk_scale": dks, "lse": lse}


def run_autograd(c, dev, core):
    """Through the autograd function of ops.temporal_attention_core / ops.spatial_attention_core."""
    x = c.qkv.to(dev, c.dtype).requires_grad_(True)
    qs, ks = c.qs.to(dev).requires_grad_(True), c.ks.to(dev).requires_grad_(True)
    y = core(x, qs, ks)
    y.backward(c.go.to(dev, c.dtype))
    torch.cuda.synchronize()
    return {"out": y.detach(), "dqkv": x.grad, "dq_scale": qs.grad, "dk_scale": ks.grad}


def run_spatial_fused(c, dev, pitched=False):
    """vvae_spatial_attn_fwd / _bwd; pitched: out and dqkv are column slices of wider buffers (ld = 3hd, ldo = hd + 64, lddq = 3hd + 64)."""
    ops = _ops()
    L = ops.lib()
    a, s, heads, d, hd, dt = c.a, c.t, c.heads, c.d, c.hd, ops.DT[c.dtype]
    pad = 64 if pitched else 0
    qkv, go = c.qkv.to(dev, c.dtype).reshape(a * s, 3 * hd), c.go.to(dev, c.dtype).reshape(a * s, hd)
    qs, ks = c.qs.to(dev), c.ks.to(dev)
    cos, sin = _tables(c, dev)
    wo, wd = _nan((a * s, hd + pad), c.dtype, dev), _nan((a * s, 3 * hd + pad), c.dtype, dev)
    out, dqkv = wo[:, :hd], wd[:, :3 * hd]
    lse2, part = _nan((a * heads, s), F32, dev), _nan((a * heads, 2, d), F32, dev)
    ops.check(L.vvae_spatial_attn_fwd(_p(qkv), 3 * hd, _p(out), hd + pad, _p(lse2), _p(qs), _p(ks), _p(cos), _p(sin), a, s, heads, d, EPS, dt,
                                      _stream()), "vvae_spatial_attn_fwd")
    ops.check(L.vvae_spatial_attn_bwd(_p(qkv), 3 * hd, _p(out), hd + pad, _p(go), hd, _p(lse2), _p(dqkv), 3 * hd + pad, _p(qs), _p(ks), _p(cos),
                                      _p(sin), _p(part), a, s, heads, d, EPS, dt, _stream()), "vvae_spatial_attn_bwd")
    dqs, dks = ops.fold_partials(part.reshape(a * heads, 2 * d), None, None, d)
    torch.cuda.synchronize()
    if pitched:
        assert bool(torch.isnan(wo[:, hd:]).all()) and bool(torch.isnan(wd[:, 3 * hd:]).all()), "a store landed beside the output columns"
    return {"out": out.reshape(a, s, hd), "dqkv": dqkv.reshape(a, s, 3 * hd), "dq_scale": dqs, "dk_scale": dks, "lse2": lse2}


def _report(route):
    for (r, what), v in sorted(FIGURES.items()):
        if r == route:
            print(f"FIGURE {route}: {what} = {v:.3e}")


def pick_lpr(t, d):
    """Lanes per row of the VALU kernels, as attn_temporal_fast.hip picks them."""
    lpr = min(4, max(1, d // 16))
    while lpr > 1 and t * lpr > 64:
        lpr //= 2
    return lpr


# =========================================================================================== GPU tests
@pytest.mark.parametrize("a,s,heads,pitched", [c + (False,) for c in SPATIAL_U] + [SPATIAL_U[2] + (True,)])
def test_spatial_fused_uniform(dev, a, s, heads, pitched):
    ops = _ops()
    c = _case("U", a, s, heads, 64, BF16, maxlen=256)
    assert ops.lib().vvae_spatial_attn_supported(s, 64, ops.DT[BF16]) == 1
    check(c, run_spatial_fused(c, dev, pitched), "spatial-fused")
    _report("spatial-fused")


@pytest.mark.parametrize("a,s,heads,copies,pitched", [c + (False,) for c in SPATIAL_H] + [SPATIAL_H[2] + (True,)])
def test_spatial_fused_onehot(dev, a, s, heads, copies, pitched):
    ops = _ops()
    c = _case("H", a, s, heads, 64, BF16, maxlen=256, copies=copies)
    assert ops.lib().vvae_spatial_attn_supported(s, 64, ops.DT[BF16]) == 1
    check(c, run_spatial_fused(c, dev, pitched), "spatial-fused")
    _report("spatial-fused")


def check_prep(c, qk, what):
    """The prep pass on one-hot inputs: scale [query codes | key codes].  bf16: those bits.  fp32 keeps the norm's 1 / sqrt(1 + eps), which
    is no fp32 power of two: every element then has the same magnitude, bit for bit, the signs are the codes', and the magnitude is
    scale / sqrt(1 + eps) at the fp32 bar."""
    want = c.prep.reshape(c.a, c.t, 2 * c.hd)
    if c.dtype == BF16:
        assert_exact(qk, want, what)
        return
    mag = qk.abs()
    assert bool((mag == mag.flatten()[0]).all()), f"{what}: the magnitudes differ, {float(mag.min())!r} .. {float(mag.max())!r}"
    assert_exact(torch.sign(qk) * c.scale, want, f"{what}: signs")
    assert_close(qk, want / math.sqrt(1.0 + EPS), rtol=F32_RTOL, atol=0.0, what=what)


def oracle_prep(c):
    q, k, _ = (z.reshape(c.a, c.t, c.heads, c.d) for z in torch.chunk(c.qkv, 3, dim=-1))
    qr, kr = OL.rope(O.layer_norm(q, c.qs, None, c.dtype), O.layer_norm(k, c.ks, None, c.dtype), c.cos, c.sin, c.dtype)
    return torch.cat([qr.reshape(c.a, c.t, c.hd), kr.reshape(c.a, c.t, c.hd)], -1)


HOST_CHECKS += [(f"prep-{i}", functools.partial(lambda mk: check_prep(mk(), oracle_prep(mk()), "oracle prep"), mk))
                for i, mk in HOST_CHECKS if i.startswith(("library-H", "prep-H"))]


@pytest.mark.parametrize("a,s,heads,d,copies", LIBRARY_H)
def test_prep_kernels_and_library_core_onehot(dev, a, s, heads, d, copies):
    """qk_prep.hip directly (bf16 and fp32), then the prep kernels around the library flash core, forward and backward."""
    ops = _ops()
    for dt in (BF16, F32):
        c = _case("H", a, s, heads, d, dt, maxlen=256, copies=copies)
        assert ops.lib().vvae_qk_prep_supported(d, ops.DT[dt]) == 1
        cos, sin = _tables(c, dev)
        qk = ops.qk_prep_fwd_raw(c.qkv.to(dev, dt), c.qs.to(dev), c.ks.to(dev), cos, sin, heads)
        check_prep(c, qk.cpu(), f"qk_prep_fwd {dt} (a {a}, s {s}, heads {heads}, d {d})")
    c = _case("H", a, s, heads, d, BF16, maxlen=256, copies=copies)
    cos, sin = _tables(c, dev)

    def core(x, qs, ks):
        assert ops.spatial_attention_supported(x, heads, 256) and ops.SPATIAL_FORCE_LIBRARY_CORE[0]
        return ops.spatial_attention_core(x, qs, ks, cos, sin, heads)
    ops.SPATIAL_FORCE_LIBRARY_CORE[0] = True
    try:
        res = run_autograd(c, dev, core)
    finally:
        ops.SPATIAL_FORCE_LIBRARY_CORE[0] = False
    check(c, res, "library-core")
    _report("library-core")


GENERIC_PARAMS = [(fam, dt, masked) + c for fam in ("U", "H") for dt in (F32, BF16) for masked in (False, True) for c in GENERIC
                  if fam == "U" or c[3] != 24]


@pytest.mark.parametrize("family,dtype,masked,a,t,heads,d", GENERIC_PARAMS)
def test_temporal_generic(dev, family, dtype, masked, a, t, heads, d):
    ops = _ops()
    c = _case(family, a, t, heads, d, dtype, "rows" if masked else "none")
    cos, sin = _tables(c, dev)
    m8 = None if c.mask_u8 is None else c.mask_u8.to(dev)

    def core(x, qs, ks):
        y = ops.temporal_attention_core(x, qs, ks, cos, sin, m8, 1, heads)
        assert y.grad_fn.args[4] is False, "the lane-per-frame kernels ran"
        return y
    ops.ATTN_FORCE_GENERIC[0] = True
    try:
        res = run_autograd(c, dev, core)
    finally:
        ops.ATTN_FORCE_GENERIC[0] = False
    check(c, res, "temporal-generic")
    _report("temporal-generic")


assert {pick_lpr(c[1], c[3]) for c in VALU if c[3] == 64} == {1, 2, 4}


@pytest.mark.parametrize("a,t,heads,d,inner,mask,mask_div", VALU)
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("family", ["U", "H"])
def test_temporal_valu(dev, family, dtype, a, t, heads, d, inner, mask, mask_div):
    """attn_temporal_fast.hip; bf16 at head_dim 64 with both matrix-core hooks off."""
    ops = _ops()
    L = ops.lib()
    c = _case(family, a, t, heads, d, dtype, mask, mask_div, inner)
    try:
        L.vvae_temporal_attn_mfma_enable(0)
        L.vvae_temporal_attn_mfma32_enable(0)
        assert L.vvae_temporal_attn_fast_supported(t, d, 3 * c.hd, c.hd, ops.DT[dtype]) == 1
        per_wg = 64 // (t * pick_lpr(t, d))
        assert L.vvae_temporal_attn_fast_blocks(a, t, heads, d, ops.DT[dtype]) == (a * heads + per_wg - 1) // per_wg
        res = run_temporal_fast(c, dev)
    finally:
        L.vvae_temporal_attn_mfma_enable(1)
        L.vvae_temporal_attn_mfma32_enable(1)
    check(c, res, "temporal-valu")
    _report("temporal-valu")


@pytest.mark.parametrize("cap", [1, 0])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("a,heads,inner", MFMA16)
@pytest.mark.parametrize("family", ["U", "H"])
def test_temporal_matrix_core_t16(dev, family, a, heads, inner, mask, cap):
    """attn_temporal_mfma.hip, the persistent grid capped at one workgroup and not at all."""
    ops = _ops()
    L = ops.lib()
    c = _case(family, a, 16, heads, 64, BF16, mask, _shared_div(a, inner), inner)
    try:
        L.vvae_temporal_attn_mfma_enable(1)
        assert L.vvae_temporal_attn_mfma_config(cap) == 0
        assert L.vvae_temporal_attn_fast_blocks(a, 16, heads, 64, ops.DT[BF16]) == (a * heads + 3) // 4     # one row per persistent wave
        res = run_temporal_fast(c, dev)
    finally:
        L.vvae_temporal_attn_mfma_config(0)
    check(c, res, "temporal-mfma16")
    _report("temporal-mfma16")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("a,t,heads", MFMA32)
@pytest.mark.parametrize("family", ["U", "H"])
def test_temporal_matrix_core_t32_t64(dev, family, a, t, heads, mask):
    """attn_temporal_mfma32.hip.  The route is held by the enable hook and by the conditions the dispatch asks for (bf16, head_dim 64,
    T 32 / 64, pitches in multiples of 8, the mask on a 4-byte boundary: run_temporal_fast), not by the partial-row count: the VALU
    kernels write one row per (sequence, head) at these shapes as well, so that count only sizes the buffer here."""
    ops = _ops()
    L = ops.lib()
    c = _case(family, a, t, heads, 64, BF16, mask, 2)
    L.vvae_temporal_attn_mfma32_enable(1)
    assert (3 * c.hd) % 8 == 0 and c.hd % 8 == 0 and c.dtype == BF16 and t in (32, 64)
    assert L.vvae_temporal_attn_fast_blocks(a, t, heads, 64, ops.DT[BF16]) == a * heads
    res = run_temporal_fast(c, dev)
    check(c, res, "temporal-mfma32")
    _report("temporal-mfma32")
