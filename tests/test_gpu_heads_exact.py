"""The encoder heads and the latent gates of csrc/encoder_head.hip, element for element, at every thread geometry of eh_dims.

The older tests of these six entry points compare tensors by relative L2 at three geometries, always hand the backward all of its
optional operands and keep u away from every decision edge.  Here the shapes alone reach the other geometries (HEAD_TABLE, GATE_TABLE),
each case asserts the one it is in from Python mirrors of eh_dims, of the two LDS sizes, of vvae_rl_gate_blocks and of the gate
launcher's nth / pieces per block, and the mirrors are held against vvae_encoder_head_ok and vvae_rl_gate_blocks on both sides of every
boundary.  A retuning then fails a test instead of shrinking coverage.

Family E, exact (ops.encoder_head, ops.encoder_head_rl, ops.encoder_head_eval).  mean: non-zero integers (+-1, +-2; the pilot token up to
16); w1 in {-1, 0, 1} with at most 64 non-zeros, w2 in {-1, 0, 1}, b1 = 1, b2 = -2; fill: multiples of 1/64 that are bf16 numbers; eps = 0.
The builder negates whole token rows so that the running dot with w2 stays small, then sets the last token (the pilot, a row of the last
trip) so that the frame's logit is exactly -3, 0 or +3.  Frames of every case: +3 / u 0.5 kept, -3 / u 0.5 dropped, 0 / u 0.5 the tie
(sigmoid = 0.5, rint half to even: dropped), 0 / u 0.75 kept, 0 / u 0.25 dropped, one masked frame (logit +3) and, at B = 3, a fully masked
sample.  Every s1 is an integer of magnitude <= 256, every partial sum of every reduction an integer (the gate sum dsg a multiple of
1/64) whose terms add up, in magnitude, to less than 2^24 granules: the order of summation cannot matter.  Upstream: dcomp small integers
(one element per tie frame is moved by at most 32 so that dsg is an integer there), dsel = -dsg on every frame but the ties (d logits is
exactly 0 there) and 4 q - dsg on them, q in {1, -2, 3}: d logits = 0.25 (dsg + dsel) = q because sigmoid'(0) = 1/4.  With gkl = None and
no gradient at log_variance, sel, comp (mean or bf16(fill) bit for bit), d mean = dcomp sel + dsi w1, d v = 0, d w1, d b1, d w2, d b2 and
d fill hold at zero tolerance.  The tie frames carry all of the selection-path gradient, the kept frames dcomp, the dropped ones d fill.
The rl flavour: every logit 0, prob = 0.5, u2 in {0.25, 0.5, 0.75} so that all four pair outcomes occur and u == prob is "dropped"; dprob2
integers whose pair sums are 4 q.  Eval, both flavours: the same frames, a mask that drops a frame of logit +3, u == prob dropped,
rint(0.5) = 0 without u, v = None.

log_variance.  v is Gaussian (sigma 8) clipped to [-30, 30] with 25, 20, -4, -4.03125, -30 and 30 planted.  Not below -30: the kernel's
d v = d lv / softplus(v) * softplus'(v) is 0 / var, and below about -88 var is 0 in bf16 (and log var = -inf in the reference as well).
The reference is the fp64 chain rounded at the kernel's two points, softplus to bf16, then log to bf16.  The kernel's softplus differs
from the fp64 one by at most K_SP = 1e-5 relative before its rounding: 2e-6 the kernel's comment grants its hardware exp, |v| 2^-24 <= 1.8e-6
for the rounded product v log2(e) in front of it, 2^-24 / log1p(e^-4) = 3.3e-6 for the rounded sum 1 + e (no more above v = -4, the series
below), 2e-6 for the hardware log or the series' remainder e^3 / 4, and a few 2^-24 of the series' own arithmetic; its log by K_LOG =
2.5e-6 (2e-6 and the rounded product with ln 2).  So the kernel's value must lie, element for element, between the smallest and the largest
of bf16(log(s) (1 -+ K_LOG)) over s in {bf16(softplus (1 - K_SP)), bf16(softplus (1 + K_SP))}: for all but the elements that sit
within K of a rounding boundary (under 0.2 % of them; the builder asserts under 3 %) the two ends are equal and the check is bit for bit.

Per-frame KL against fp64 on the kernel's own log_variance.  Every term 0.5 (e^lv - 1 - lv + mu^2) is non-negative; with M = 0.5 (e^lv + 1
+ |lv| + mu^2) the magnitudes that enter it, the kernel's value is off by at most (D + 49) 2^-24 sum M (scaled as the KL is): 40 for the
hardware exp (2e-6 and its argument), 5 for the roundings inside a term, D = 8 trips + 6 + 16 + 1 for the additions along the deepest path
(a thread's own elements, the butterfly, the waves), 4 for the scaling.  The builder asserts that this is below half of the smallest
token's contribution in every unmasked frame.  Masked frames and the fully masked sample (seq_len clamped to 1) give exactly 0.

Family G, generic (the Gaussian inputs of test_gpu_fused_vs_oracle.py, eps != 0, a KL gradient, a gradient at log_variance), every output
and gradient element for element against plain fp64 evaluated from the kernel's own log_variance and selection (parameters as the bf16
numbers the kernel reads; no rounding in between).  Derived: comp within 2^-8 |z| (its rounding) + 4e-6 |eps| sigma + 2^-23 (|mu| + |eps|
sigma) (the hardware exp and two fp32 roundings), as an absolute bound, so a cancelling mu + eps sigma is no exemption; dropped frames are
bf16(fill) bit for bit; d fill within (trips + TY + frames) 2^-24 sum |dcomp| (fp32 additions, any order of that depth); log_variance
and the per-frame KL as in Family E (a Gaussian token comes arbitrarily close to a contribution of 0, so the builder asserts the KL
bound below half of the average token's here, of the smallest token's in Family E).  Not derived
(the bf16 roundings of s1, the logit, d logits and d s1 act through sigmoid'): d mean, d v, d w1, d b1, d w2, d b2 are held to MARGIN = 4
times the worst ratio of the fp32 CPU restatement's error to a unit, the unit being 2^-8 times the sum of the magnitudes of the element's
terms (one bf16 rounding of each); a CPU ratio below 1 counts as 1, since one rounding of d logits is what any correct kernel may differ by.
The bar never comes from the kernel's output.  Parameter gradients are also checked per frame (one frame alone gets an upstream gradient,
so the folded sum is that frame's partial row) and, at (16, 96), with every operand of the backward absent in turn, gkl with strides (1, 0)
and (T, 1), and one mask row shared by all samples.

rl gate (ops.rl_gate, and vvae_rl_gate_bwd for its d fill partial rows): integer z and dcomp, bf16 fill: comp, mask, dz, every partial row
(summed over exactly the pieces the mirror gives the block) and d fill at zero tolerance.

Every builder validates its case on the CPU before a GPU result is looked at; tests/test_host.py runs the builders (HOST_CHECKS) and
feeds the assertions CPU results with one defect each (DEFECT_CHECKS): every one of them must raise.

Bit for bit against the parent of the commit that gave the three head kernels one prologue, one phase A and one launch path:
tests/golden/heads_parent_bits.json holds dtype, shape and SHA-256 of every forward output, gradient and per-frame partial row of both
flavours at four geometries, of the operand combinations and of the eval forms, recorded on the GPU from the commit before
(tests/golden/make_heads_parent_bits.py).  Family G's six measured bars allow a rounding; this test allows none.
"""
import collections
import ctypes
import functools
import importlib.util
import json
import math
import os
import sys
import types
import zlib

import pytest
import torch

from util import assert_exact, ints, rnd

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U24, R8 = 2.0 ** -24, 2.0 ** -8
K_SP, K_LOG = 1e-5, 2.5e-6
MARGIN = 4.0
EXACT = 2 ** 24


class _Case(types.SimpleNamespace):
    """A case: hashable by identity, so that the bars measured for it can be cached."""
    __hash__ = object.__hash__


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31 - 1000)


def _bf(x):
    """x rounded to bf16, in x's dtype."""
    return x.float().bfloat16().to(x.dtype)


def _cdiv(a, b):
    return -(-a // b)


def _lib():
    from video_vae_amd._lib import lib
    return lib()


def _ops():
    from video_vae_amd import ops
    return ops


def _within(got, want64, tol, what, name):
    """|got - want| <= tol element for element (0 where no rounding is allowed); a NaN never passes.  -> the largest error / bound."""
    assert tuple(got.shape) == tuple(want64.shape), (what, name, tuple(got.shape), tuple(want64.shape))
    err = (got.detach().double().cpu() - want64.double()).abs()
    tol = torch.as_tensor(tol, dtype=F64).expand(err.shape)
    bad = ~(err <= tol)
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err != 0, float("inf"), 0.0).double())
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    if bool(bad.any()):
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        raise AssertionError(f"{what}: {name}: {int(bad.sum())}/{bad.numel()} elements outside the bound, worst error / bound {worst:.3e}; first at "
                             f"{i}: got {float(got[i])!r} want {float(want64[i])!r} bound {float(tol[i]):.3e}; last at {tuple(idx[-1].tolist())}")
    return worst


def _exact(got, want64, what, name):
    assert_exact(got.detach().cpu(), want64.reshape(got.shape), f"{what}: {name}")


def _bits(got, want, what, name):
    """bf16 tensors, bit for bit."""
    g, w = got.detach().cpu(), want.to(BF16).reshape(got.shape)
    assert g.dtype == BF16, (what, name, g.dtype)
    bad = g.view(torch.int16) != w.view(torch.int16)
    bad &= ~((g == 0) & (w == 0))
    if bool(bad.any()):
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        raise AssertionError(f"{what}: {name}: {int(bad.sum())}/{bad.numel()} elements differ bit for bit; first at {i}: got {float(g[i])!r} "
                             f"want {float(w[i])!r}; last at {tuple(idx[-1].tolist())}")


def _figure(what, name, value):
    print(f"FIGURE {what}: {name}: error / bound = {value:.3e}")


# =========================================================================================== the dispatch, mirrored
EH_MAX_THREADS, EH_MAX_HW, EH_MAX_LD, LDS_LIMIT = 1024, 4096, 1024, 64 * 1024


def eh_regime(hw, ld):
    """eh_dims and the two LDS sizes of encoder_head.hip -> CG, TY, threads launched and active, trips of the token loop, rows in the
    last trip, ok or refused."""
    r = types.SimpleNamespace(ok=False, shape_ok=False)
    if hw <= 0 or hw > EH_MAX_HW or hw % 4 or ld <= 0 or ld > EH_MAX_LD or ld % 8:
        return r
    r.shape_ok = True
    r.cg = ld // 8
    r.ty = min(EH_MAX_THREADS // r.cg, hw)
    r.active = r.cg * r.ty
    r.threads = _cdiv(r.active, 64) * 64
    r.trips = _cdiv(hw, r.ty)
    r.last = hw - (r.trips - 1) * r.ty
    r.lds_fwd, r.lds_bwd = (hw + hw * r.cg + 20) * 4, (hw + r.ty * ld + 20) * 4
    r.ok = r.lds_fwd <= LDS_LIMIT and r.lds_bwd <= LDS_LIMIT
    return r


# (HW, LD): CG, TY, threads, active threads, trips, rows in the last trip, ok; what the row is there for
HEAD_TABLE = {(4, 8): (1, 4, 64, 4, 1, 4, True, "one wavefront with 4 active threads, one trip"),
              (16, 96): (12, 16, 192, 192, 1, 16, True, "TY = HW, 192 threads, one trip"),
              (256, 96): (12, 85, 1024, 1020, 4, 1, True, "production: 1020 of 1024 threads, 4 trips, 1 row in the last"),
              (1256, 96): (12, 85, 1024, 1020, 15, 66, True, "the largest HW the forward's LDS admits at LD = 96, 15 trips"),
              (1260, 96): (12, 85, 1024, 1020, 15, 70, False, "the first HW refused at LD = 96"),
              (4096, 8): (1, 1024, 1024, 1024, 4, 1024, True, "CG = 1, TY = 1024, 4 full trips, EH_MAX_HW"),
              (124, 1024): (128, 8, 1024, 1024, 16, 4, True, "CG = 128, TY = 8, 15.5 trips, EH_MAX_LD"),
              (128, 1024): (128, 8, 1024, 1024, 16, 8, False, "refused by the LDS bound at LD = 1024"),
              (100, 200): (25, 40, 1024, 1000, 3, 20, True, "CG = 25, TY = 40, 1000 of 1024 threads, 2.5 trips")}
OK_SHAPES = [s for s, row in HEAD_TABLE.items() if row[6]]
REFUSED_SHAPES = [s for s, row in HEAD_TABLE.items() if not row[6]]
T_FRAMES = 3


def claimed_head(hw, ld):
    """The regime of a row of HEAD_TABLE, asserted from the mirror and held against the library."""
    r = eh_regime(hw, ld)
    row = HEAD_TABLE[(hw, ld)]
    assert (r.cg, r.ty, r.threads, r.active, r.trips, r.last, r.ok) == row[:7], ((hw, ld), vars(r), row[7], "eh_dims moved: re-derive the shapes")
    assert bool(_lib().vvae_encoder_head_ok(2, T_FRAMES, hw, ld)) == r.ok, ((hw, ld), "the mirror of the LDS bound no longer matches the library")
    r.what = row[7]
    return r


def gate_regime(b2, t, per, ld):
    """vvae_rl_gate_blocks and the launchers of the rl gate -> block rows per clip (and whether the cap cut them), threads, pieces per
    block, the piece range of every block of a clip, the forward's grid and its sweeps."""
    r = types.SimpleNamespace()
    clips = b2 // 2
    r.pieces = t * (per // 8)
    want = _cdiv(r.pieces, 2048)
    cap = 2048 // max(clips, 1)
    r.capped = want > cap
    r.nbx = max(cap, 1) if r.capped else want
    r.wanted = want
    r.rows = r.nbx * clips
    cg = ld // 8
    r.nth = 256 // cg * cg
    r.ppb = _cdiv(_cdiv(r.pieces, r.nbx), r.nth) * r.nth
    r.ranges = [(min(i * r.ppb, r.pieces), min((i + 1) * r.ppb, r.pieces)) for i in range(r.nbx)]
    r.last = r.ranges[-1][1] - r.ranges[-1][0]
    all_pieces = b2 * t * (per // 8)
    r.fwd_blocks = min(_cdiv(all_pieces, 256), 4096)
    r.fwd_sweeps = _cdiv(all_pieces, r.fwd_blocks * 256)
    return r


def gate_blocks(b2, t, per):
    if b2 <= 0 or t <= 0 or per <= 0:
        return 0
    return gate_regime(b2, t, per, 8).rows


# (clips, T, HW, LD): blocks per clip, threads, pieces per block, pieces of the last block, capped, forward blocks, forward sweeps; what for
GATE_TABLE = {(2, 3, 16, 96): (1, 252, 756, 576, False, 9, 1, "one block per clip, 252 threads"),
              (2, 3, 100, 8): (1, 256, 512, 300, False, 5, 1, "LD = 8: cg = 1, 256 threads"),
              (2, 2, 760, 96): (9, 252, 2268, 96, False, 285, 1, "9 blocks per clip, the last with 96 pieces for 252 threads"),
              (2, 3, 272, 200): (10, 250, 2250, 150, False, 319, 1, "LD = 200: 250 threads, the last block with 150 pieces"),
              (1, 2, 4, 2048): (1, 256, 2048, 2048, False, 16, 1, "LD = 2048: cg = 256, one channel group per thread"),
              (2, 3, 3500, 200): (129, 250, 2250, 0, False, 4096, 2, "past the forward's 4096-block cap: a second sweep; the last 12 blocks of a clip get no piece"),
              (512, 1, 8200, 8): (4, 256, 2304, 1288, True, 4096, 9, "past the vvae_rl_gate_blocks cap: 5 blocks per clip cut to 4")}
GATE_SMALL = [s for s in GATE_TABLE if s[0] * s[1] * s[2] * s[3] < 10 ** 7]
GATE_CAPPED = (512, 1, 8200, 8)


def claimed_gate(clips, t, hw, ld):
    r = gate_regime(2 * clips, t, hw * ld, ld)
    row = GATE_TABLE[(clips, t, hw, ld)]
    assert (r.nbx, r.nth, r.ppb, r.last, r.capped, r.fwd_blocks, r.fwd_sweeps) == row[:7], ((clips, t, hw, ld), vars(r), row[7])
    assert _lib().vvae_rl_gate_blocks(2 * clips, t, hw * ld) == r.rows, "the mirror of vvae_rl_gate_blocks no longer matches the library"
    assert _lib().vvae_rl_gate_ok(2 * clips, t, hw * ld, ld) == 1
    assert r.ranges[0][0] == 0 and r.ranges[-1][1] == r.pieces and all(a[1] == b[0] for a, b in zip(r.ranges, r.ranges[1:]))
    r.what = row[7]
    return r


def _mirrors_match_the_library():
    lib = _lib()
    for hw, ld in HEAD_TABLE:
        claimed_head(hw, ld)
    lds = (8, 16, 96, 104, 200, 512, 1016, 1024, 1032, 12, 0)
    for ld in lds:
        hws = {4, 6, 8, 16, 100, 124, 128, 252, 256, 1024, 4092, 4096, 4100, 0}
        if eh_regime(4, ld).shape_ok:                                     # both sides of this LD's LDS boundary
            top = max((h for h in range(4, EH_MAX_HW + 1, 4) if eh_regime(h, ld).ok), default=None)
            assert top is not None
            hws |= {top - 4, top, top + 4}
            assert top == EH_MAX_HW or not eh_regime(top + 4, ld).ok
        for hw in sorted(hws):
            assert bool(lib.vvae_encoder_head_ok(2, T_FRAMES, hw, ld)) == eh_regime(hw, ld).ok, (hw, ld)
    assert eh_regime(1256, 96).lds_fwd == (1256 * 13 + 20) * 4 <= LDS_LIMIT < eh_regime(1260, 96).lds_fwd
    assert not lib.vvae_encoder_head_ok(0, 3, 16, 96) and not lib.vvae_encoder_head_ok(2, 0, 16, 96)
    for key in GATE_TABLE:
        claimed_gate(*key)
    for b2 in (2, 4, 6, 64, 1024, 2048, 4096, 4098):
        for t in (1, 3, 16):
            for per in (8, 1536, 16384, 16392, 24576, 65600, 262144, 2 ** 22 + 8):
                assert lib.vvae_rl_gate_blocks(b2, t, per) == gate_blocks(b2, t, per), (b2, t, per)
    assert lib.vvae_rl_gate_blocks(0, 3, 1536) == 0 and lib.vvae_rl_gate_blocks(4, 0, 1536) == 0
    assert lib.vvae_rl_gate_ok(4, 3, 4 * 2048, 2048) == 1 and lib.vvae_rl_gate_ok(4, 3, 4 * 2056, 2056) == 0


# =========================================================================================== the heads in torch: fp32 restatement and fp64
Cfg = collections.namedtuple("Cfg", "present only gkl shared_mask", defaults=(("dcomp", "dsel"), None, "sample", False))
CFG_E = Cfg()
CFG_G = Cfg(("dcomp", "dsel", "gkl", "dlv"))


def head_math(k, cfg, restate, lv_in=None, sel_in=None, defect=None):
    """The forward and backward of a case.  restate: in fp32 with the kernel's bf16 rounding points (the CPU restatement); else in fp64
    without them, from ``lv_in`` (log_variance) and ``sel_in`` (model: the selection; rl: the frame masks), the reference.  ``defect``: one
    of the mistakes of DEFECT_CHECKS.  -> outputs, gradients, the per-frame partial rows and the units of the measured bars."""
    dt = F32 if restate else F64
    q = _bf if restate else (lambda x: x)
    b, t, hw, ld = k.shape
    rl = k.flavour == "rl"
    m, v, eps = k.mean.to(dt), k.v.to(dt), k.eps.to(dt)
    w1b, w2b, b1b, b2b = (_bf(x).to(dt) for x in (k.w1, k.w2, k.b1, k.b2))
    fr = (k.fill if defect == "fill-unrounded" else _bf(k.fill)).to(dt)
    mask = (k.mask[:1] if cfg.shared_mask else k.mask).to(dt).expand(b, t)
    tok = torch.ones(hw, dtype=dt)
    if defect == "row-dropped":                                          # the one row of the last trip that only the last token lane reads
        tok[hw - 1] = 0.0
    s1 = q((m * w1b).sum(-1) + b1b)
    logits = q(q((s1 * w2b).sum(-1) + b2b) + 1.0)
    var = _bf(torch.where(v > 20, v, torch.log1p(torch.exp(v))))
    lv = q(torch.log(var)) if lv_in is None else lv_in.to(dt)
    if rl and lv_in is not None:
        lv = lv.view(b, 2, t, hw, ld)[:, 0]
    sig, elv = torch.exp(0.5 * lv), torch.exp(lv)
    z = m + eps * sig
    den = (mask.sum(1).clamp_min(1.0) * float(t) * float(hw) * float(ld))[:, None]
    klsum = (0.5 * (elv - 1.0 - lv + m * m) * tok[:, None]).sum((2, 3))
    mk = mask.clone()
    if defect == "dead-kl":
        mk[mask.sum(1) == 0] = 1.0
    klf = klsum * mk / den
    res, tz = {}, tok[:, None]
    one = torch.ones(b, t, dtype=dt)
    if cfg.only is not None:
        one = torch.zeros(b, t, dtype=dt)
        one[cfg.only] = 1.0
    gkl = dlv = None
    if "gkl" in cfg.present:
        gkl = (k.gkl_b[:, None].expand(-1, t) if cfg.gkl == "sample" else k.gkl_bt).to(dt) * (one.repeat_interleave(2, 0) if rl else one)
    if defect == "null-present":
        gkl = torch.ones(2 * b if rl else b, t, dtype=dt)
    if "dlv" in cfg.present:
        dlv = k.dlv.to(dt) * (one.repeat_interleave(2, 0) if rl else one)[:, :, None, None]
    dcomp = k.dcomp.to(dt) * (one.repeat_interleave(2, 0) if rl else one)[:, :, None, None] if "dcomp" in cfg.present else None
    dsel = k.dsel.to(dt).view(-1, t) * (one.repeat_interleave(2, 0) if rl else one) if "dsel" in cfg.present else None
    if not rl:
        uc = k.u.to(dt).clamp(1e-20, 1.0 - 1e-20)
        y = logits + torch.log(uc / (1.0 - uc))
        sg = 1.0 / (1.0 + torch.exp(-y))
        sel = torch.round(sg)
        if defect == "tie-up":
            sel = torch.where(sg == 0.5, torch.ones_like(sel), sel)
        if sel_in is not None:
            sel = sel_in.reshape(b, t).to(dt)
        keep = sel[:, :, None, None]
        comp = torch.where(keep != 0, z, fr.expand_as(z))
        res.update(lv=lv, comp=comp, sel=sel.view(b, t, 1, 1), kl=klf, y=y)
        zero = torch.zeros_like(z)
        dc = dcomp if dcomp is not None else zero
        dsg = (dc * (z - fr) * tz).sum((2, 3))
        dl = q((dsg + (dsel if dsel is not None else 0.0)) * sg * (1.0 - sg))
        dck, dfa = dc * keep, dc * (1.0 - keep)
        ks = gkl * mask / den if gkl is not None else torch.zeros(b, t, dtype=dt)
        dx = dlv if dlv is not None else zero
    else:
        sg = 1.0 / (1.0 + torch.exp(-logits))
        prob = q(sg)
        u2 = k.u.to(dt).view(b, 2, t)
        keep2 = (u2 <= prob[:, None]) if defect == "u-eq-kept" else (u2 < prob[:, None])
        if sel_in is not None:
            keep2 = sel_in.reshape(b, 2, t) != 0
        kf = keep2.to(dt)[..., None, None]
        comp2 = torch.where(kf != 0, z[:, None], fr.expand_as(z)[:, None])
        if defect == "pair-swapped":
            comp2 = comp2.flip(1)
        dbl = lambda x: x.repeat_interleave(2, 0)
        res.update(lv=dbl(lv), mean2=dbl(m), comp=comp2.reshape(2 * b, t, hw, ld), sel=dbl(prob).view(2 * b, t, 1, 1),
                   mask2=keep2.to(dt).reshape(2 * b, t, 1, 1), kl=dbl(klf), y=logits)
        zero = torch.zeros_like(z)
        d2 = dcomp.view(b, 2, t, hw, ld) if dcomp is not None else torch.zeros(b, 2, t, hw, ld, dtype=dt)
        dck, dfa = (d2 * kf).sum(1), (d2 * (1.0 - kf)).sum(1)
        dl = q((dsel.view(b, 2, t).sum(1) if dsel is not None else torch.zeros(b, t, dtype=dt)) * sg * (1.0 - sg))
        ks = gkl.view(b, 2, t).sum(1) * mask / den if gkl is not None else torch.zeros(b, t, dtype=dt)
        dx = q(dlv.view(b, 2, t, hw, ld).sum(1)) if dlv is not None else zero
    dsi = q(dl[..., None] * w2b)
    ks4, dsi4 = ks[:, :, None, None], dsi[..., None]
    dm = (dck + ks4 * m + dsi4 * w1b) * tz
    dsp = torch.where(v > 20, torch.ones_like(v), 1.0 / (1.0 + torch.exp(-v)))
    terms_lv = (dck * eps * 0.5 * sig, ks4 * 0.5 * (elv - 1.0), dx)
    dvv = (terms_lv[0] + terms_lv[1] + terms_lv[2]) / var * dsp * tz
    if defect == "row-dropped":
        res["comp"] = res["comp"] * tz
    if defect == "cg-swapped":                                           # channel group 0 written where group 1 belongs and back
        perm = torch.arange(ld)
        perm[:16] = torch.cat([torch.arange(8, 16), torch.arange(0, 8)])
        res["comp"], dm = res["comp"][..., perm], dm[..., perm]
    rows = {"p1": (m * dsi4 * tz).sum(2), "p2": s1 * dl[..., None], "p3": (dfa * tz).sum(2), "pb1": (dsi * tok).sum(-1), "pb2": dl}
    res.update(dmean=dm, dv=dvv, dw1=rows["p1"].sum((0, 1)), db1=rows["pb1"].sum().reshape(1), dw2=rows["p2"].sum((0, 1)),
               db2=rows["pb2"].sum().reshape(1), dfill=rows["p3"].sum((0, 1)))
    if restate:
        for name in ("lv", "comp", "dmean", "dv", "mean2"):
            if name in res:
                res[name] = res[name].to(BF16)
        res = {n: (x if x.dtype == BF16 else x.float()) for n, x in res.items()}
    else:
        unit = {"dmean": R8 * (dck.abs() + (ks4 * m).abs() + (dsi4 * w1b).abs()), "dv": R8 * sum(x.abs() for x in terms_lv) / var * dsp,
                "dw1": R8 * (m * dsi4).abs().sum((0, 1, 2)), "db1": R8 * dsi.abs().sum().reshape(1), "dw2": R8 * (s1 * dl[..., None]).abs().sum((0, 1)),
                "db2": R8 * dl.abs().sum().reshape(1)}
        res["unit"] = unit
        res["z"], res["sig"], res["dfa_abs"] = z, sig, (dfa.abs() if not rl else (d2.abs() * (1.0 - kf)).sum(1)).sum((0, 1, 2))
        res["klM"] = (0.5 * (elv + 1.0 + lv.abs() + m * m)).sum((2, 3)) * mask / den
    return res


MEASURED = ("dmean", "dv", "dw1", "db1", "dw2", "db2")
GRADS = MEASURED + ("dfill",)


def lv_interval(v):
    """Where the kernel's log_variance may lie, element for element (see the module docstring) -> lo, hi (fp64 holding bf16 numbers)."""
    x = v.double()
    s = torch.where(x > 20, x, torch.log1p(torch.exp(x)))
    cands = []
    for ks in (1.0 - K_SP, 1.0 + K_SP):
        l = torch.log(torch.where(x > 20, x, _bf(s * ks)))
        cands += [_bf(l * (1.0 - K_LOG)), _bf(l * (1.0 + K_LOG))]
    c = torch.stack(cands)
    return c.min(0).values, c.max(0).values


def kl_depth(r):
    return 8 * r.trips + 6 + 16 + 1 + 49


@functools.lru_cache(maxsize=64)
def _bars(k, cfg):
    """MARGIN x the worst error / unit of the fp32 CPU restatement against fp64 on its own log_variance and selection, per output."""
    cpu = head_math(k, cfg, True)
    ref = head_math(k, cfg, False, cpu["lv"], cpu["mask2"] if k.flavour == "rl" else cpu["sel"])
    bars, ratios = {}, {}
    for name in MEASURED:
        err, unit = (cpu[name].double() - ref[name]).abs(), ref["unit"][name]
        assert bool((err[unit == 0] == 0).all()), name
        ratios[name] = float((err / unit.clamp_min(1e-300))[unit > 0].max()) if bool((unit > 0).any()) else 0.0
        assert ratios[name] < 16.0, (name, ratios[name], "the CPU restatement is further from fp64 than any rounding explains")
        bars[name] = MARGIN * max(ratios[name], 1.0)
    return bars, ratios


def check_head(k, res, route, cfg=None):
    """Every assertion of a case on the outputs and gradients of one forward + backward; a route may return a part of them."""
    cfg = cfg or k.cfg
    b, t, hw, ld = k.shape
    rl = k.flavour == "rl"
    what = f"{route} {k.family} {k.flavour} (HW {hw}, LD {ld}, B {b}{', ' + k.note if k.note else ''}{'' if cfg == k.cfg else ', ' + str(cfg)})"
    for name, x in res.items():
        if torch.is_tensor(x):
            bad = int((~torch.isfinite(x.double())).sum())
            assert bad == 0, f"{what}: {name}: {bad}/{x.numel()} elements are not finite"
    lv = res["lv"].detach().cpu()
    lo, hi = k.lv_lo, k.lv_hi
    if rl:
        assert torch.equal(lv[0::2], lv[1::2]), f"{what}: log_variance: the members of a pair differ"
        assert torch.equal(res["mean2"][0::2].cpu(), res["mean2"][1::2].cpu()), f"{what}: mean2: the members of a pair differ"
        _bits(res["mean2"][0::2], k.mean, what, "mean2")
        assert torch.equal(res["sel"][0::2].cpu(), res["sel"][1::2].cpu()), f"{what}: probability: the members of a pair differ"
        assert torch.equal(res["kl"][0::2].cpu(), res["kl"][1::2].cpu()), f"{what}: kl: the members of a pair differ"
        lo, hi = lo.repeat_interleave(2, 0), hi.repeat_interleave(2, 0)
    off = (lv.double() < lo) | (lv.double() > hi) | lv.double().isnan()
    if bool(off.any()):
        i = tuple(off.nonzero()[0].tolist())
        raise AssertionError(f"{what}: log_variance: {int(off.sum())}/{off.numel()} elements outside [lo, hi]; first at {i}: got {float(lv[i])!r}, "
                             f"[{float(lo[i])!r}, {float(hi[i])!r}]; last at {tuple(off.nonzero()[-1].tolist())}")
    gate = res["mask2"] if rl else res["sel"]
    if k.family == "E":
        _exact(gate, k.want["mask2" if rl else "sel"], what, "mask2" if rl else "sel")
        if rl:
            _exact(res["sel"], torch.full((2 * b, t, 1, 1), 0.5, dtype=F64), what, "probability")
    else:
        _exact(gate, k.gate64, what, "mask2" if rl else "sel")
    ref = head_math(k, cfg, False, lv, gate.detach().cpu())
    # per-frame KL on the kernel's own log_variance
    tol = kl_depth(k.r) * U24 * ref["klM"]
    dead = (k.mask[:1] if cfg.shared_mask else k.mask).expand(b, t) == 0
    if rl:
        tol, dead = tol.repeat_interleave(2, 0), dead.repeat_interleave(2, 0)
    _figure(what, "kl", _within(res["kl"], ref["kl"], tol, what, "kl"))
    assert float(res["kl"].detach().cpu()[dead].abs().max()) == 0.0, f"{what}: kl: a masked frame is not exactly 0"
    if k.family == "E":
        _bits(res["comp"], k.want["comp"], what, "comp")
        for name in GRADS:
            if name in res:
                _exact(res[name], k.want[name], what, name)
        return
    keepf = (gate.detach().cpu().double() != 0).reshape(-1, t, 1, 1)
    intr = 4e-6 * (k.eps.double().abs() * ref["sig"]) + 2.0 ** -23 * (k.mean.double().abs() + (k.eps.double() * ref["sig"]).abs())
    ztol = R8 * (ref["z"].abs() + intr) + intr
    if rl:
        ztol = ztol.repeat_interleave(2, 0)
    _figure(what, "comp", _within(res["comp"], ref["comp"], torch.where(keepf, ztol, torch.zeros_like(ztol)), what, "comp"))
    if "dmean" not in res:
        return
    bars, _ = _bars(k, cfg)
    for name in MEASURED:
        worst = _within(res[name].reshape(ref[name].shape), ref[name], bars[name] * ref["unit"][name], what, name)
        print(f"FIGURE {what}: {name}: worst error / unit {worst * bars[name]:.3f}, bar {bars[name]:.3f}")
    depth = (2 if rl else 1) * k.r.trips + k.r.ty + b * t
    _figure(what, "dfill", _within(res["dfill"].reshape(ld), ref["dfill"], depth * U24 * ref["dfa_abs"], what, "dfill"))


# =========================================================================================== Family E: cases
def frame_plan(b, rl):
    """-> the logit each frame is built to have, its u (model) and the mask: (b, 3) each."""
    tgt = [[3.0, -3.0, 0.0], [0.0, 0.0, 3.0], [0.0, 3.0, -3.0]][:b]
    u = [[0.5, 0.5, 0.5], [0.75, 0.25, 0.5], [0.5, 0.5, 0.5]][:b]
    mask = [[1.0, 1.0, 1.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]][:b]
    tgt = torch.tensor(tgt, dtype=F64)
    return (torch.zeros_like(tgt) if rl else tgt), torch.tensor(u), torch.tensor(mask)


def _planted_v(shape, seed):
    v = _bf((rnd(shape, seed) * 8.0).clamp(-30.0, 30.0))
    plant = torch.tensor([25.0, 20.0, -4.0, -4.03125, -30.0, 30.0])
    v.view(-1)[:6] = plant
    v.view(-1)[-6:] = plant.flip(0)
    assert bool((_bf(v) == v).all()) and float(v.min()) == -30.0 and float(v.max()) == 30.0
    return v


def _kl_separates(k, cfg, smallest=True):
    """The KL bound is below half of the smallest token's contribution in every unmasked frame (Family G, whose Gaussian tokens come
    arbitrarily close to a contribution of 0: of the average token's)."""
    cpu = head_math(k, cfg, True)
    lv = cpu["lv"].double()
    ref = head_math(k, cfg, False, lv, cpu["mask2"] if k.flavour == "rl" else cpu["sel"])
    if k.flavour == "rl":
        lv = lv[0::2]
    b, t, hw, ld = k.shape
    tokens = (0.5 * (torch.exp(lv) - 1.0 - lv + k.mean.double() ** 2)).sum(3)
    tokens = tokens.min(2).values if smallest else tokens.mean(2)                                   # (b, t)
    mask = k.mask.double().expand(b, t)
    den = (mask.sum(1).clamp_min(1.0) * t * hw * ld)[:, None]
    live = mask != 0
    bound = kl_depth(k.r) * U24 * ref["klM"]
    assert bool((bound < 0.5 * tokens * mask / den)[live].all()), ("the KL bound no longer separates one token", k.shape,
                                                                 float((bound / (tokens * mask / den).clamp_min(1e-300))[live].max()))


@functools.lru_cache(maxsize=16)
def e_case(flavour, hw, ld, fillkind="bf16"):
    k = _Case()
    rl = flavour == "rl"
    k.family, k.flavour, k.cfg, k.note = "E", flavour, CFG_E, "" if fillkind == "bf16" else "fill no bf16 number"
    k.r = claimed_head(hw, ld)
    assert k.r.ok
    t = T_FRAMES
    b = 3 if 9 * hw * ld < 10 ** 6 else 2
    k.shape, frames = (b, t, hw, ld), b * t
    assert frames * hw * ld < 10 ** 6
    seed = _seed("E", hw, ld)
    shape = k.shape
    tgt, u, k.mask = frame_plan(b, rl)
    k.tgt = tgt
    # ---- parameters
    nz = min(64, ld - ld // 4)
    g = torch.Generator().manual_seed(seed)
    pos = torch.randperm(ld, generator=g)[:nz].sort().values
    k.w1 = torch.zeros(ld)
    k.w1[pos] = ints((nz,), seed + 1, 0, 1) * 2.0 - 1.0
    k.w2 = ints((hw,), seed + 2, -1, 1)
    k.w2[hw - 1] = 1.0
    k.b1, k.b2 = torch.tensor([1.0]), torch.tensor([-2.0])
    fill = ints((ld,), seed + 3, -64, 64) / 64.0
    fill[0], fill[ld - 1] = 33.0 / 64.0, 1.0 / 64.0
    assert bool((_bf(fill) == fill).all())
    k.fill = fill if fillkind == "bf16" else fill * (1.0 + 2.0 ** -10)
    assert bool((_bf(k.fill) == fill).all()) and (fillkind == "bf16" or bool((k.fill != fill)[fill != 0].all()))
    # ---- mean: token rows negated so that the running dot with w2 stays small, then the pilot token
    mean = (ints(shape, seed + 4, 1, 2) * (ints(shape, seed + 5, 0, 1) * 2.0 - 1.0)).view(frames, hw, ld)
    a = (mean.double() * k.w1.double()).sum(-1)
    tot = torch.zeros(frames, dtype=F64)
    b1, b2 = float(k.b1), float(k.b2)
    for j in range(hw - 1):
        w = float(k.w2[j])
        if w == 0.0:
            continue
        cp, cm = (a[:, j] + b1) * w, (-a[:, j] + b1) * w
        neg = (tot + cm).abs() < (tot + cp).abs()
        mean[neg, j] = -mean[neg, j]
        tot += torch.where(neg, cm, cp)
    need = (tgt.view(frames) - 1.0 - b2) - tot - b1                      # what the pilot's dot with w1 must be
    half = nz // 2
    assert nz % 2 == 0 and half >= 2
    prod = torch.ones(frames, nz, dtype=F64)
    prod[:, 1::2] = -1.0
    qq, rr = torch.div(need.abs(), half, rounding_mode="floor"), need.abs() % half
    add = qq[:, None] + (torch.arange(half)[None, :] < rr[:, None]).double()
    prod[:, 0::2] += torch.where(need[:, None] > 0, add, torch.zeros_like(add))
    prod[:, 1::2] -= torch.where(need[:, None] < 0, add, torch.zeros_like(add))
    mean[:, hw - 1, pos] = (prod * k.w1[pos].double()).float()
    k.mean = mean.view(shape)
    assert bool((k.mean != 0).all()) and float(k.mean.abs().max()) <= 16 and bool((_bf(k.mean) == k.mean).all())
    s1 = (k.mean.double() * k.w1.double()).sum(-1) + b1
    assert float(s1.abs().max()) <= 256 and bool((s1 == s1.round()).all())
    assert float((s1 * k.w2.double()).abs().sum(-1).max()) < EXACT
    assert torch.equal((s1 * k.w2.double()).sum(-1) + b2 + 1.0, tgt), "the pilot token did not land the logit"
    k.v, k.eps = _planted_v(shape, seed + 6), torch.zeros(shape)
    k.lv_lo, k.lv_hi = lv_interval(k.v)
    k.lv_loose = float((k.lv_lo != k.lv_hi).double().mean())
    assert k.lv_loose < 0.03, k.lv_loose
    amp = 2 if hw * ld <= 32768 else 1
    m64, f64 = k.mean.double(), fill.double()
    w2d, w1d = k.w2.double(), k.w1.double()
    k.want = {}
    if not rl:
        k.u = u
        tie = (tgt == 0) & (u == 0.5)
        sel = ((tgt > 0) | ((tgt == 0) & (u > 0.5))).double()
        assert int(tie.sum()) >= 1 and sorted(set(zip(tgt.view(-1).tolist(), u.view(-1).tolist()))) == [(-3.0, 0.5), (0.0, 0.25), (0.0, 0.5), (0.0, 0.75), (3.0, 0.5)]
        dc = ints(shape, seed + 7, -amp, amp).double()
        resid = torch.round(64.0 * (dc * f64).sum((2, 3))) % 64              # dsg must be an integer on the tie frames
        delta = -(((resid + 32) % 64) - 32)
        dc[:, :, 0, ld - 1] += torch.where(tie, delta, torch.zeros_like(delta))
        dsg = (dc * (m64 - f64)).sum((2, 3))
        assert bool((dsg[tie] == dsg[tie].round()).all()) and float((dc.abs() * (m64 - f64).abs()).sum((2, 3)).max()) * 64 < EXACT
        quarter = torch.tensor([1.0, -2.0, 3.0], dtype=F64)[torch.arange(frames) % 3].view(b, t)
        dl = torch.where(tie, quarter, torch.zeros_like(quarter))
        dsel = torch.where(tie, 4.0 * quarter, torch.zeros_like(quarter)) - dsg
        assert bool((dsel.float().double() == dsel).all()) and bool((dsel[tie] == dsel[tie].round()).all())
        k.dcomp, k.dsel = dc.float(), dsel.float().view(b, t, 1, 1)
        keep = sel[:, :, None, None]
        k.want.update(sel=sel.view(b, t, 1, 1), comp=torch.where(keep != 0, m64, f64.expand_as(m64)))
        dck, dfa = dc * keep, dc * (1.0 - keep)
    else:
        pairs = torch.tensor([[0.25, 0.25], [0.25, 0.5], [0.75, 0.25], [0.5, 0.75]])       # kept/kept, kept/dropped, dropped/kept, dropped/dropped
        u2 = pairs[torch.arange(frames) % 4].view(b, t, 2).permute(0, 2, 1).reshape(2 * b, t)
        k.u = u2.contiguous()
        keep2 = (u2 < 0.5).double().view(b, 2, t)
        assert len(set(map(tuple, keep2.permute(0, 2, 1).reshape(-1, 2).tolist()))) == 4 and bool((u2 == 0.5).any())
        d2 = ints((2 * b, t, hw, ld), seed + 7, -amp, amp).double()
        quarter = torch.tensor([1.0, -2.0, 3.0, 0.0], dtype=F64)[torch.arange(frames) % 4].view(b, t)
        first = ints((b, t), seed + 8, -5, 5).double()
        dprob = torch.stack([first, 4.0 * quarter - first], 1).reshape(2 * b, t)
        k.dcomp, k.dsel = d2.float(), dprob.float().view(2 * b, t, 1, 1)
        dl = quarter
        kf = keep2[..., None, None]
        d2v = d2.view(b, 2, t, hw, ld)
        dck, dfa = (d2v * kf).sum(1), (d2v * (1.0 - kf)).sum(1)
        k.want.update(mask2=keep2.reshape(2 * b, t, 1, 1), comp=torch.where(kf != 0, m64[:, None], f64.expand_as(m64)[:, None]).reshape(2 * b, t, hw, ld))
    assert bool((_bf(k.dcomp) == k.dcomp).all()) and float(k.dcomp.abs().max()) <= 34
    dsi = dl[..., None] * w2d
    k.want.update(dmean=dck + dsi[..., None] * w1d, dv=torch.zeros(shape, dtype=F64), dw1=(m64 * dsi[..., None]).sum((0, 1, 2)), db1=dsi.sum().reshape(1),
                  dw2=(s1 * dl[..., None]).sum((0, 1)), db2=dl.sum().reshape(1), dfill=dfa.sum((0, 1, 2)))
    assert bool((_bf(k.want["dmean"]) == k.want["dmean"]).all()), "d mean is no bf16 tensor"
    for terms in (m64 * dsi[..., None], s1 * dl[..., None], dfa, dck):
        assert float(terms.abs().sum()) < EXACT and bool((terms == terms.round()).all())
    assert float(k.want["dw1"].abs().max()) > 0 and float(k.want["dw2"].abs().max()) > 0 and float(k.want["dfill"].abs().max()) > 0
    # ---- the fp64 evaluation reproduces the closed forms; the CPU restatement passes the assertions
    cpu = head_math(k, k.cfg, True)
    ref = head_math(k, k.cfg, False, cpu["lv"], k.want["mask2" if rl else "sel"])
    for name in GRADS:
        assert torch.equal(ref[name].reshape(k.want[name].shape), k.want[name]), name
    _kl_separates(k, k.cfg)
    check_head(k, cpu, "cpu")
    return k


# =========================================================================================== Family G: cases
@functools.lru_cache(maxsize=12)
def g_case(flavour, hw, ld, draw=0):
    """The inputs of test_gpu_fused_vs_oracle.py::test_encoder_head_vs_oracle / _rl_vs_oracle, with a gradient at log_variance.  ``draw``:
    another seed for a geometry whose first draw puts a frame at a decision edge (the builder refuses such a case)."""
    k = _Case()
    rl = flavour == "rl"
    k.family, k.flavour, k.cfg, k.note = "G", flavour, CFG_G, ""
    k.r = claimed_head(hw, ld)
    b, t = 2, T_FRAMES
    k.shape = shape = (b, t, hw, ld)
    g = torch.Generator().manual_seed(_seed("G", flavour, hw, ld, *([draw] if draw else [])))
    rn = lambda *s: torch.randn(*s, generator=g)
    k.mean, k.v = _bf(rn(*shape) * 0.5), _bf(rn(*shape) * 1.5)
    k.w1, k.b1, k.w2, k.b2 = rn(ld) * ld ** -0.5, rn(1) * 0.1, rn(hw) * hw ** -0.5, rn(1) * 0.1
    k.fill, k.eps = rn(ld) * 0.02, rn(*shape)
    k.mask = torch.ones(b, t)
    k.mask[0, -1] = 0.0
    b2 = 2 * b if rl else b
    if rl:      # uniforms far from any selection probability (sigmoid(1 + O(0.3)) ~ 0.7): 0.05 keeps the frame, 0.97 drops it
        k.u = torch.where(torch.rand(b2, t, generator=g) < 0.6, torch.full((), 0.05), torch.full((), 0.97))
        k.u[0, 0], k.u[1, 0] = 0.05, 0.97
    else:       # far from the gate's threshold
        r = torch.rand(b, t, generator=g)
        k.u = torch.where(torch.rand(b, t, generator=g) < 0.5, 0.02 + 0.08 * r, 0.9 + 0.08 * r)
        k.u.view(-1)[0], k.u.view(-1)[-1] = 0.02, 0.98
    k.dcomp, k.dsel = _bf(rn(b2, t, hw, ld)), rn(b2, t, 1, 1)
    k.gkl_b, k.gkl_bt, k.dlv = rn(b2), rn(b2, t), _bf(rn(b2, t, hw, ld) * 0.1)
    k.lv_lo, k.lv_hi = lv_interval(k.v)
    cpu = head_math(k, k.cfg, True)
    ref = head_math(k, k.cfg, False)
    if rl:
        y = ref["y"]
        prob = 1.0 / (1.0 + torch.exp(-y))
        assert float((k.u.double().view(b, 2, t) - prob[:, None]).abs().min()) > 0.05
    else:
        assert float(ref["y"].abs().min()) > 0.25, "a frame sits at the decision edge"
    k.gate64 = ref["mask2" if rl else "sel"]
    assert 0 < float(k.gate64.sum()) < k.gate64.numel() and torch.equal(cpu["mask2" if rl else "sel"].double(), k.gate64)
    _kl_separates(k, k.cfg, smallest=False)
    check_head(k, cpu, "cpu")
    return k


COMBOS = [Cfg(("dcomp",)), Cfg(("dsel",)), Cfg(("gkl",)), Cfg(("dlv",)), Cfg(("dsel", "gkl", "dlv")), Cfg(("dcomp", "dsel", "gkl", "dlv"), None, "frame"),
          Cfg(("dcomp", "dsel", "gkl", "dlv"), None, "sample", True)]
PER_FRAME = [Cfg(("dcomp", "dsel", "gkl", "dlv"), only, "frame") for only in ((0, 1), (1, 2))]


def _cfg_id(c):
    return "+".join(c.present) + ("" if c.only is None else f"-only{c.only[0]}{c.only[1]}") + ("" if c.gkl == "sample" else "-gklTx1") + ("-sharedmask" if c.shared_mask else "")


# =========================================================================================== eval: cases
EVAL_FORMS = [("model", "nomask"), ("model", "mask"), ("rl", "u"), ("rl", "nou"), ("rl", "u-mask"), ("model", "nov")]


def eval_inputs(k, flavour, form):
    """-> u (b, t) or None, mask (b, t) or None, whether v is given, for one form of ops.encoder_head_eval on the Family E model case."""
    b, t = k.shape[:2]
    u = None
    if form.startswith("u"):
        p3 = float(_bf(torch.tensor(1.0 / (1.0 + math.exp(-3.0)))))          # bf16(sigmoid(3)): u == prob there is "dropped"
        pick = {(3.0, 0.5): p3, (-3.0, 0.5): 0.01, (0.0, 0.5): 0.5, (0.0, 0.75): 0.75, (0.0, 0.25): 0.25}
        u = torch.tensor([pick[(float(a), float(c))] for a, c in zip(k.tgt.view(-1), k.u.view(-1))]).view(b, t)
        u[1, 2] = 0.1                                                       # the masked frame of logit +3: kept but for the mask
    mask = k.mask if form.endswith("mask") and form != "nomask" else None
    return u, mask, form != "nov"


def eval_math(k, flavour, form, defect=None):
    """encoder_head_eval_kernel in fp64 on a Family E case (every value on the selection path is exact) -> comp, sel, prob."""
    b, t, hw, ld = k.shape
    u, mask, _ = eval_inputs(k, flavour, form)
    sg = 1.0 / (1.0 + torch.exp(-k.tgt))
    prob = None
    if flavour == "rl":
        prob = _bf(sg)
        sel = (u.double() < prob).double() if u is not None else torch.round(prob)
    else:
        sel = torch.round(sg)
    if mask is not None and defect != "masked-kept":
        sel = sel * (mask.double() != 0)
    comp = torch.where(sel[:, :, None, None] != 0, k.mean.double(), _bf(k.fill).double().expand(k.shape))
    return {"comp": comp, "sel": sel, "prob": prob}


def check_eval(k, res, flavour, form, route):
    what = f"{route} eval {flavour} {form} (HW {k.shape[2]}, LD {k.shape[3]}{', ' + k.note if k.note else ''})"
    want = eval_math(k, flavour, form)
    _exact(res["sel"], want["sel"], what, "sel")
    _bits(res["comp"], want["comp"], what, "comp")
    if flavour == "rl":
        _exact(res["prob"], want["prob"], what, "prob")
    else:
        assert res["prob"] is None
    if form == "nov":
        assert res["lv"] is None, f"{what}: a log_variance without v"
    else:
        lv = res["lv"].detach().cpu().double()
        assert bool(((lv >= k.lv_lo) & (lv <= k.lv_hi)).all()), f"{what}: log_variance outside [lo, hi]"
    kinds = {"model": {"nomask": [1, 0, 0, 0, 0, 1], "mask": [1, 0, 0, 0, 0, 0], "nov": [1, 0, 0, 0, 0, 1]},
             "rl": {"u": [0, 1, 0, 0, 1, 1], "nou": [1, 0, 0, 0, 0, 1], "u-mask": [0, 1, 0, 0, 1, 0]}}[flavour][form]
    assert want["sel"].view(-1)[:6].tolist() == [float(x) for x in kinds], (what, "the case no longer holds the frame kinds it is there for")


def _eval_host(hw, ld):
    k = e_case("model", hw, ld)
    for flavour, form in EVAL_FORMS:
        want = eval_math(k, flavour, form)
        check_eval(k, {"comp": want["comp"].to(BF16), "sel": want["sel"].float(), "prob": want["prob"], "lv": None if form == "nov" else k.lv_lo.to(BF16)},
                   flavour, form, "cpu")


# =========================================================================================== rl gate: cases
def gate_case(clips, t, hw, ld, device="cpu"):
    """Integer z and dcomp, a bf16 fill, prob in {0.25, 0.5, 0.75} and u from the same set: u == prob occurs and is "dropped"."""
    k = types.SimpleNamespace()
    k.key, k.r = (clips, t, hw, ld), claimed_gate(clips, t, hw, ld)
    g = torch.Generator(device=device).manual_seed(_seed("gate", clips, t, hw, ld))
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g, device=device, dtype=torch.int8)
    k.z = ri((clips, t, hw, ld), -3, 3).float()
    k.dcomp = ri((2 * clips, t, hw, ld), -2, 2).to(BF16)
    levels = torch.tensor([0.25, 0.5, 0.75], device=device)
    k.prob = levels[ri((clips, t), 0, 2).long()]
    k.u = levels[ri((2 * clips, t), 0, 2).long()]
    k.u[0, 0], k.u[1, 0], k.prob[0, 0] = 0.5, 0.25, 0.5                   # u == prob next to u < prob in one pair
    k.fill = (ri((ld,), -64, 64).float() / 64.0)
    assert bool((_bf(k.fill) == k.fill).all())
    keep = k.u.view(clips, 2, t) < k.prob[:, None]
    assert 0 < int(keep.sum()) < keep.numel()
    kf = keep[..., None, None]
    k.mask = keep.reshape(2 * clips, t, 1, 1).float()
    k.comp = torch.where(kf, k.z[:, None], k.fill.expand_as(k.z)[:, None]).reshape(2 * clips, t, hw, ld).to(BF16)
    d2 = k.dcomp.float().view(clips, 2, t, hw, ld)
    k.dz = (d2 * kf).sum(1)
    dropped = (d2 * ~kf).sum(1).view(clips, t * hw * ld)
    k.part = torch.stack([dropped[:, lo * 8:hi * 8].reshape(clips, -1, ld).sum(1) for lo, hi in k.r.ranges], 1).reshape(k.r.rows, ld)
    k.dfill = k.part.sum(0)
    assert float((d2.abs() * ~kf).sum(1).view(clips, -1, ld).sum((0, 1)).max()) < EXACT, "the d fill sums leave the exact range of fp32"
    check_gate(k, cpu_gate(k), "cpu")
    return k


_gate_case_cpu = functools.lru_cache(maxsize=2)(gate_case)


def cpu_gate(k, defect=None):
    """What the case expects, as a result; ``defect`` "part-row-missing": the last block of the last clip never writes its d fill row,
    "u-eq-kept": u <= prob."""
    part = k.part.clone()
    res = {"comp": k.comp, "mask": k.mask, "dz": k.dz}
    if defect == "part-row-missing":
        part[-1] = 0.0
    if defect == "u-eq-kept":
        clips, t = k.prob.shape
        res["mask"] = (k.u.view(clips, 2, t) <= k.prob[:, None]).reshape(k.mask.shape).float()
    res["part"], res["dfill"] = part, part.sum(0)
    return res


def check_gate(k, res, route):
    what = f"{route} rl gate {k.key}: {k.r.what}"
    same = lambda a, b: torch.equal(a.detach().to(b.device), b)
    assert same(res["mask"], k.mask), f"{what}: mask: {int((res['mask'].to(k.mask.device) != k.mask).sum())} frames differ"
    assert same(res["comp"].view(torch.int16), k.comp.view(torch.int16)) or same(res["comp"].float(), k.comp.float()), f"{what}: comp is not bit for bit"
    assert same(res["dz"], k.dz), f"{what}: dz: {int((res['dz'].to(k.dz.device) != k.dz).sum())} elements differ"
    if "part" in res:
        bad = (res["part"].to(k.part.device) != k.part).any(1)
        assert not bool(bad.any()), f"{what}: d fill partial rows {bad.nonzero().view(-1).tolist()[:8]} of {k.r.rows} differ"
    assert same(res["dfill"].reshape(-1), k.dfill), f"{what}: d fill differs"


# =========================================================================================== host and defect checks (tests/test_host.py)
E_CASES = [("model", hw, ld, "bf16") for hw, ld in OK_SHAPES] + [("model", 16, 96, "unrounded")] + [("rl", hw, ld, "bf16") for hw, ld in OK_SHAPES]
G_CASES = [("model", hw, ld) for hw, ld in OK_SHAPES] + [("rl", hw, ld) for hw, ld in ((16, 96), (256, 96), (100, 200))]


def _combos_host():
    k = g_case("model", 16, 96)
    for cfg in COMBOS + PER_FRAME:
        check_head(k, head_math(k, cfg, True), "cpu", cfg)
    k = g_case("model", 256, 96)
    for cfg in PER_FRAME:
        check_head(k, head_math(k, cfg, True), "cpu", cfg)


def _host_checks():
    cs = [("mirrors", _mirrors_match_the_library)]
    cs += [(f"E-{f}-HW{hw}-LD{ld}-{fk}", functools.partial(e_case, f, hw, ld, fk)) for f, hw, ld, fk in E_CASES]
    cs += [(f"G-{f}-HW{hw}-LD{ld}", functools.partial(g_case, f, hw, ld)) for f, hw, ld in G_CASES]
    cs += [("G-operand-combinations", _combos_host)]
    cs += [(f"eval-HW{hw}-LD{ld}", functools.partial(_eval_host, hw, ld)) for hw, ld in OK_SHAPES]
    cs += [("gate-" + "x".join(map(str, key)), functools.partial(_gate_case_cpu, *key)) for key in GATE_SMALL]
    cs += [("gate-capped-regime", functools.partial(claimed_gate, *GATE_CAPPED))]
    return cs


def _raises(fn, match):
    with pytest.raises(AssertionError, match=match):
        fn()


def _head_defect(family, flavour, hw, ld, fillkind, defect, name):
    k = e_case(flavour, hw, ld, fillkind) if family == "E" else g_case(flavour, hw, ld)
    if defect is None:
        return check_head(k, head_math(k, k.cfg, True), "cpu")
    _raises(lambda: check_head(k, head_math(k, k.cfg, True, defect=defect), "cpu"), rf"\): {name}: ")


def _eval_defect():
    k = e_case("model", 16, 96)
    for flavour, form in (("model", "mask"), ("rl", "u-mask")):
        bad = eval_math(k, flavour, form, "masked-kept")
        res = {"comp": bad["comp"].to(BF16), "sel": bad["sel"].float(), "prob": bad["prob"], "lv": k.lv_lo.to(BF16)}
        _raises(lambda: check_eval(k, res, flavour, form, "cpu"), r"\): sel: ")


def _gate_defect(key, defect, name):
    k = _gate_case_cpu(*key)
    _raises(lambda: check_gate(k, cpu_gate(k, defect), "cpu"), name)


def _defect_checks():
    out = []
    for hw, ld in ((256, 96), (100, 200)):
        out.append((f"E-model-HW{hw}-clean", functools.partial(_head_defect, "E", "model", hw, ld, "bf16", None, None)))
        out.append((f"E-model-HW{hw}-row-dropped", functools.partial(_head_defect, "E", "model", hw, ld, "bf16", "row-dropped", "kl")))
        out.append((f"E-model-HW{hw}-cg-swapped", functools.partial(_head_defect, "E", "model", hw, ld, "bf16", "cg-swapped", "comp")))
        out.append((f"E-model-HW{hw}-tie-up", functools.partial(_head_defect, "E", "model", hw, ld, "bf16", "tie-up", "sel")))
        out.append((f"E-model-HW{hw}-null-present", functools.partial(_head_defect, "E", "model", hw, ld, "bf16", "null-present", "dmean")))
        out.append((f"E-model-HW{hw}-dead-kl", functools.partial(_head_defect, "E", "model", hw, ld, "bf16", "dead-kl", "kl")))
        out.append((f"E-rl-HW{hw}-u-eq-kept", functools.partial(_head_defect, "E", "rl", hw, ld, "bf16", "u-eq-kept", "mask2")))
        out.append((f"E-rl-HW{hw}-pair-swapped", functools.partial(_head_defect, "E", "rl", hw, ld, "bf16", "pair-swapped", "comp")))
        out.append((f"E-rl-HW{hw}-dead-kl", functools.partial(_head_defect, "E", "rl", hw, ld, "bf16", "dead-kl", "kl")))
        out.append((f"G-model-HW{hw}-row-dropped", functools.partial(_head_defect, "G", "model", hw, ld, None, "row-dropped", "kl")))
        out.append((f"G-model-HW{hw}-cg-swapped", functools.partial(_head_defect, "G", "model", hw, ld, None, "cg-swapped", "comp")))
    out.append(("E-model-fill-unrounded", functools.partial(_head_defect, "E", "model", 16, 96, "unrounded", "fill-unrounded", "dmean")))
    out.append(("eval-masked-kept", _eval_defect))
    out.append(("gate-part-row-missing", functools.partial(_gate_defect, (2, 2, 760, 96), "part-row-missing", "d fill partial rows")))
    out.append(("gate-u-eq-kept", functools.partial(_gate_defect, (2, 3, 16, 96), "u-eq-kept", "mask: ")))
    return out


HOST_CHECKS = _host_checks()
DEFECT_CHECKS = _defect_checks()


# =========================================================================================== GPU runners
def _poison(dev, nbytes):
    """Fill the allocator's free blocks of an output's size with NaN bit patterns, so that an element no kernel wrote cannot pass on what
    an earlier run left there.  Best effort, no proof."""
    blocks = [torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


def _leaves(k, dev):
    b, t, hw, ld = k.shape
    vals = (k.mean.to(dev, BF16), k.v.to(dev, BF16), k.w1.view(ld, 1).to(dev), k.b1.to(dev), k.w2.view(hw, 1).to(dev), k.b2.to(dev),
            k.fill.view(1, 1, 1, ld).to(dev))
    return [x.clone().requires_grad_(True) for x in vals]


def run_head(k, dev, cfg=None):
    """ops.encoder_head / ops.encoder_head_rl forward, then torch.autograd.grad on exactly the outputs ``cfg`` names: the others reach the
    backward kernel as NULL."""
    cfg = cfg or k.cfg
    ops = _ops()
    b, t, hw, ld = k.shape
    rl = k.flavour == "rl"
    b2 = 2 * b if rl else b
    _poison(dev, b2 * t * hw * ld * 2)
    leaves = _leaves(k, dev)
    assert ops.encoder_head_ok(*leaves)
    mask = (k.mask[:1] if cfg.shared_mask else k.mask).to(dev)
    res = {}
    if rl:
        lv, mean2, comp, sel, mask2, kl = ops.encoder_head_rl(*leaves, k.u.view(b2, t, 1, 1).to(dev), k.eps.to(dev), mask)
        res.update(mean2=mean2, mask2=mask2)
    else:
        lv, comp, sel, kl = ops.encoder_head(*leaves, k.u.view(b, t, 1).to(dev), k.eps.to(dev), mask)
    res.update(lv=lv, comp=comp, sel=sel, kl=kl)
    one = torch.ones(b2, t, device=dev)
    if cfg.only is not None:
        one = torch.zeros(b, t, device=dev)
        one[cfg.only] = 1.0
        one = one.repeat_interleave(2, 0) if rl else one
    outs, gos, seen = [], [], []
    if "dcomp" in cfg.present:
        outs.append(comp); gos.append((k.dcomp.to(dev) * one[:, :, None, None]).to(BF16))
    if "dsel" in cfg.present:
        outs.append(sel); gos.append(k.dsel.to(dev) * one[:, :, None, None])
    if "gkl" in cfg.present:
        g = k.gkl_b.to(dev)[:, None].expand(b2, t) if cfg.gkl == "sample" else (k.gkl_bt.to(dev) * one).contiguous()
        if cfg.gkl == "sample" and cfg.only is not None:
            g = (k.gkl_b.to(dev)[:, None] * one).contiguous()
        kl.register_hook(lambda gr: seen.append(gr.stride()))
        outs.append(kl); gos.append(g)
    if "dlv" in cfg.present:
        outs.append(lv); gos.append((k.dlv.to(dev) * one[:, :, None, None]).to(BF16))
    grads = torch.autograd.grad(outs, leaves, gos)
    torch.cuda.synchronize()
    if "gkl" in cfg.present and cfg.only is None:
        assert seen == [(1, 0) if cfg.gkl == "sample" else (t, 1)], (seen, "the KL gradient did not reach the backward with the strides meant")
    for name, g in zip(("dmean", "dv", "dw1", "db1", "dw2", "db2", "dfill"), grads):
        res[name] = g.reshape(-1) if name not in ("dmean", "dv") else g
    return {n: x.detach().cpu() for n, x in res.items()}


def run_eval(k, dev, flavour, form):
    ops = _ops()
    u, mask, with_v = eval_inputs(k, flavour, form)
    leaves = [x.detach() for x in _leaves(k, dev)]
    assert ops.encoder_head_eval_ok(leaves[0], *leaves[2:])
    _poison(dev, k.mean.numel() * 2)
    with torch.no_grad():
        lv, comp, sel, prob = ops.encoder_head_eval(leaves[0], leaves[1] if with_v else None, *leaves[2:], u=None if u is None else u.to(dev),
                                                    mask_bt=None if mask is None else mask.to(dev), rl=flavour == "rl")
    torch.cuda.synchronize()
    cpu = lambda x: None if x is None else x.cpu()
    return {"lv": cpu(lv), "comp": cpu(comp), "sel": cpu(sel), "prob": cpu(prob)}


def run_gate(k, dev):
    """ops.rl_gate forward and backward, then vvae_rl_gate_bwd once more on raw buffers for the d fill partial rows the op folds away."""
    ops, lib = _ops(), _lib()
    clips, t, hw, ld = k.key
    z, fill = k.z.to(dev).requires_grad_(True), k.fill.view(1, 1, 1, ld).to(dev).requires_grad_(True)
    assert ops.rl_gate_ok(z, k.prob.to(dev), fill)
    _poison(dev, 2 * z.numel() * 2)
    comp, mask = ops.rl_gate(z, k.prob.to(dev), k.u.view(2 * clips, t, 1, 1).to(dev), fill)
    dcomp = k.dcomp.to(dev)
    dz, dfill = torch.autograd.grad([comp], [z, fill], [dcomp])
    rows = lib.vvae_rl_gate_blocks(2 * clips, t, hw * ld)
    assert rows == k.r.rows
    part = torch.full((rows + 1, ld), float("nan"), device=dev)
    dz2 = torch.empty_like(dz)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    code = lib.vvae_rl_gate_bwd(vp(dcomp), vp(mask), vp(dz2), vp(part), 2 * clips, t, hw * ld, ld, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == 0 and bool(part[rows].isnan().all()), "vvae_rl_gate_bwd failed or wrote past its partial rows"
    assert torch.equal(dz2, dz)
    return {"comp": comp.detach(), "mask": mask.detach(), "dz": dz, "dfill": dfill.reshape(-1), "part": part[:rows]}


# =========================================================================================== GPU tests
def test_mirrors_match_the_library():
    _mirrors_match_the_library()


@pytest.mark.parametrize("flavour,hw,ld,fillkind", E_CASES, ids=[f"{f}-HW{hw}-LD{ld}-{fk}" for f, hw, ld, fk in E_CASES])
def test_heads_exact_selection_path(dev, flavour, hw, ld, fillkind):
    """ops.encoder_head / ops.encoder_head_rl forward and backward on Family E at a row of HEAD_TABLE: zero tolerance but for
    log_variance (its derived interval) and the KL (its derived bound)."""
    k = e_case(flavour, hw, ld, fillkind)
    assert k.r.ok and (k.r.cg, k.r.ty, k.r.threads, k.r.active, k.r.trips, k.r.last) == HEAD_TABLE[(hw, ld)][:6], k.r.what
    print(f"REGIME (HW {hw}, LD {ld}): {k.r.what}; log_variance elements with lo < hi: {k.lv_loose:.4f}")
    check_head(k, run_head(k, dev), "gpu")


@pytest.mark.parametrize("hw,ld", OK_SHAPES, ids=[f"HW{hw}-LD{ld}" for hw, ld in OK_SHAPES])
def test_eval_heads_exact(dev, hw, ld):
    """ops.encoder_head_eval in both flavours on the Family E frames: with and without a mask, with u (u == prob is dropped) and without
    (rint(0.5) = 0), without v; comp bit for bit."""
    k = e_case("model", hw, ld)
    assert k.r.ok, k.r.what
    results = {}
    for flavour, form in EVAL_FORMS:
        results[form] = run_eval(k, dev, flavour, form)
        check_eval(k, results[form], flavour, form, "gpu")
    assert torch.equal(results["nov"]["comp"].view(torch.int16), results["nomask"]["comp"].view(torch.int16)), "comp changes when v is left out"


def test_eval_heads_unrounded_fill(dev):
    """A fill token that is no bf16 number: dropped frames hold bf16(fill) bit for bit."""
    k = e_case("model", 16, 96, "unrounded")
    for flavour, form in EVAL_FORMS:
        check_eval(k, run_eval(k, dev, flavour, form), flavour, form, "gpu")


@pytest.mark.parametrize("hw,ld", REFUSED_SHAPES, ids=[f"HW{hw}-LD{ld}" for hw, ld in REFUSED_SHAPES])
def test_heads_refuse_what_the_lds_cannot_hold(dev, hw, ld):
    """The first shape past the LDS bound: the ok predicates say no, and the entry points return an error before any launch."""
    from video_vae_amd._lib import VvaeError
    ops = _ops()
    r = claimed_head(hw, ld)
    assert r.shape_ok and not r.ok and r.lds_fwd > LDS_LIMIT, r.what
    b, t = 1, 2
    mean = torch.zeros(b, t, hw, ld, dtype=BF16, device=dev)
    params = [torch.zeros(ld, 1, device=dev), torch.zeros(1, device=dev), torch.zeros(hw, 1, device=dev), torch.zeros(1, device=dev),
              torch.zeros(1, 1, 1, ld, device=dev)]
    assert not ops.encoder_head_ok(mean, mean, *params) and not ops.encoder_head_eval_ok(mean, *params)
    with pytest.raises(VvaeError):
        ops.encoder_head(mean, mean, *params, torch.full((b, t, 1), 0.5, device=dev), torch.zeros_like(mean, dtype=F32), torch.ones(b, t, device=dev))
    with pytest.raises(VvaeError):
        ops.encoder_head_rl(mean, mean, *params, torch.full((2 * b, t, 1, 1), 0.5, device=dev), torch.zeros_like(mean, dtype=F32), torch.ones(b, t, device=dev))
    with pytest.raises(VvaeError):
        ops.encoder_head_eval(mean, mean, *params)
    torch.cuda.synchronize()


@pytest.mark.parametrize("flavour,hw,ld", G_CASES, ids=[f"{f}-HW{hw}-LD{ld}" for f, hw, ld in G_CASES])
def test_heads_generic_per_element(dev, flavour, hw, ld):
    """Family G with every operand of the backward present: each output and gradient element for element against fp64."""
    k = g_case(flavour, hw, ld)
    assert k.r.ok and (k.r.cg, k.r.ty, k.r.trips, k.r.last) == tuple(HEAD_TABLE[(hw, ld)][i] for i in (0, 1, 4, 5)), k.r.what
    check_head(k, run_head(k, dev), "gpu")


@pytest.mark.parametrize("cfg", COMBOS, ids=[_cfg_id(c) for c in COMBOS])
def test_heads_backward_operand_combinations(dev, cfg):
    """(16, 96): one upstream gradient at a time, all but dcomp, gkl contiguous with strides (T, 1), one mask row for all samples."""
    k = g_case("model", 16, 96)
    check_head(k, run_head(k, dev, cfg), "gpu", cfg)


@pytest.mark.parametrize("hw,ld", [(16, 96), (256, 96)], ids=["HW16-LD96", "HW256-LD96"])
@pytest.mark.parametrize("cfg", PER_FRAME, ids=[_cfg_id(c) for c in PER_FRAME])
def test_heads_parameter_gradients_per_frame(dev, hw, ld, cfg):
    """One frame alone gets upstream gradients: the folded parameter gradients are that frame's partial rows of part1, part2, part3, partb."""
    k = g_case("model", hw, ld)
    res = run_head(k, dev, cfg)
    check_head(k, res, "gpu", cfg)
    assert float(res["dw1"].abs().max()) > 0 and float(res["dw2"].abs().max()) > 0


@pytest.mark.parametrize("key", GATE_SMALL, ids=["x".join(map(str, key)) for key in GATE_SMALL])
def test_rl_gate_exact(dev, key):
    k = _gate_case_cpu(*key)
    print(f"REGIME rl gate {key}: {k.r.what}")
    check_gate(k, run_gate(k, dev), "gpu")


def test_rl_gate_past_the_block_cap(dev):
    """512 clips of 8200 x 8: vvae_rl_gate_blocks wants 5 block rows per clip and its cap of 2048 in all leaves 4.  Case and reference are
    built on the device (67 M dcomp elements)."""
    k = gate_case(*GATE_CAPPED, device=dev)
    assert k.r.capped and k.r.wanted == 5 and k.r.nbx == 4 and k.r.rows == 2048, k.r.what
    check_gate(k, run_gate(k, dev), "gpu")


def test_heads_bit_for_bit_with_the_parent(dev):
    """Every member of tests/golden/heads_parent_bits.json (make_heads_parent_bits.py: forward outputs, gradients and per-frame partial rows
    of both flavours at (4, 8), (16, 96), (100, 200), (256, 96), the operand combinations and the eval forms at (16, 96)), recorded on the
    GPU before the head kernels shared their prologue, phase A and launch path: same dtype, same shape, same bytes."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_heads_parent_bits", os.path.join(golden, "make_heads_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = mod.describe(mod.record(sys.modules[__name__], dev))
    with open(os.path.join(golden, "heads_parent_bits.json")) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want) and len(want) > 350, (len(got), len(want), sorted(set(got) ^ set(want))[:8])
    bad = [f"{m}: got {got[m]}, recorded {want[m]}" for m in sorted(want) if got[m] != want[m]]
    assert not bad, f"{len(bad)} of {len(want)} members differ from what the parent computed; first: {bad[0]}; all: {[b.split(':')[0] for b in bad]}"
