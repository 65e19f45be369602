"""Write-through output stores (csrc/common.hpp: buf_store16_wt, 16 bytes per lane through a buffer descriptor, sc1).  The kernels that
store this way: gemm_pp.hip (the plain product, + residual and the SiLU pair: epilogues 0, 1, 2), layernorm.hip (forward and backward),
gn_silu.hip (gn_silu_fwd_kernel) and attn_spatial.hip (both cores).  The stores move no value, so every check is a coverage check: each
output element is written, with the value the reference gives, and nothing next to the output is touched -- a descriptor's range check
must neither drop a row nor reach a neighbour.  Cases that run kernels left on plain stores are marked below: they hold the same
property for the unchanged code and exercise none of the new stores.

  * gemm_pp against gemm_nt.hip (``form="nt"``), bitwise, all four epilogues (epilogue 3, x silu', stores plainly), at the smallest
    shapes that reach each store path (one tile per workgroup: the final epilogue only; two tiles: a mid-launch and a final epilogue),
    into a column slice of a wider buffer pre-filled with a NaN bit pattern (ldc = N + 64, the same for the saved pre-activation);
  * the hand-over through kernel boundaries inside a replayed graph, gemm_pp -> layer_norm -> gemm_pp(res=...), eight replays with fresh
    inputs, bitwise against the same chain run eagerly on the nt form: a consumer that reads stale or unwritten lines fails here;
  * LayerNorm forward (plain and with the fused residual add) and backward (with and without the skip gradient), GroupNorm + SiLU
    (forward: write-through; forward with the pool and backward: plain stores) and the spatial attention cores: NaN pre-fill with
    guard rows / columns around every output, two runs bitwise equal, and the torch formula or the oracle at the tolerances of the
    kernel's tests in tests/test_gpu_ops.py.
"""
import pytest
import torch

from util import assert_close, assert_close_scaled, rnd

PATTERN = 0x7FC5                                   # a bf16 NaN no kernel here produces
PATTERN32 = 0x7FC00A5A                             # the same for fp32


def _ops():
    from video_vae_amd import ops
    return ops


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _patterned(dev, rows, cols):
    return torch.full((rows, cols), PATTERN, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------ gemm_pp
#           M      N     K    tiles per workgroup
PP_SHAPES = [(256, 192, 128),        # one 256 x 192 tile
             (512, 128, 192),        # two workgroups, one 256 x 128 tile each
             (8192, 2048, 128),      # 512 tiles of 256 x 128 on 256 workgroups: mid-launch and final epilogues
             (16384, 1536, 128)]     # 512 tiles of 256 x 192


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", PP_SHAPES)
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_gemm_pp_fills_a_column_slice_and_nothing_else(dev, m, n, k, epi):
    ops = _ops()
    a = rnd((m, k), 501).to(dev, torch.bfloat16)
    b = (rnd((n, k), 502) / k ** 0.5).to(dev, torch.bfloat16)
    bias = rnd((n,), 503).to(dev) if epi != 3 else None
    res = rnd((m, n), 504, 2.0).to(dev, torch.bfloat16) if epi in (1, 3) else None
    want = ops.gemm_nt(a, b, bias, res, epi, form="nt")
    want = want if epi == 2 else (want, None)

    ldc = n + 64
    assert ops.lib().vvae_gemm_pp_supported(m, n, k, k, k, ldc) == 1
    wide = [_patterned(dev, m + 2, ldc) for _ in range(2 if epi == 2 else 1)]      # a guard row above and below, 32 + 32 guard columns
    outs = [w[1:m + 1, 32:32 + n] for w in wide]
    c, c2 = outs[0], (outs[1] if epi == 2 else None)
    ops.check(ops.lib().vvae_gemm_pp_bf16(_p(a), k, _p(b), k, _p(c), ldc, _p(bias), _p(res), n if res is not None else 0, _p(c2), ldc, epi,
                                          m, n, k, _stream()), "vvae_gemm_pp_bf16")
    torch.cuda.synchronize()
    for w, o, ref, what in zip(wide, outs, want, ("output", "saved pre-activation")):
        assert torch.equal(_bits(o), _bits(ref)), f"{what}: {int((_bits(o) != _bits(ref)).sum())} of {o.numel()} elements differ from gemm_nt"
        outside = torch.ones_like(w, dtype=torch.bool)
        outside[1:m + 1, 32:32 + n] = False
        assert bool((_bits(w)[outside] == PATTERN).all()), f"{what}: a store landed outside the column slice"


@pytest.mark.gpu
def test_chain_through_kernel_boundaries_in_a_replayed_graph(dev):
    ops = _ops()
    m, n = 512, 768
    w1 = (rnd((n, n), 511) / n ** 0.5).to(dev, torch.bfloat16)
    w2 = (rnd((n, n), 512) / n ** 0.5).to(dev, torch.bfloat16)
    b1, b2 = rnd((n,), 513).to(dev), rnd((n,), 514).to(dev)
    gam, bet = (1 + 0.2 * rnd((n,), 515)).to(dev), (0.1 * rnd((n,), 516)).to(dev)
    x = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)
    r = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)

    def chain(form):
        h = ops.gemm_nt(x, w1, b1, form=form)
        y = ops.layer_norm(h, gam, bet)
        return ops.gemm_nt(y, w2, b2, r, ops.EPI_RES, form=form)

    st = torch.cuda.Stream()
    with torch.cuda.stream(st), torch.no_grad():
        chain("pp")                                            # warm: function attributes are set outside the capture
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            out = chain("pp")
        for i in range(8):
            x.copy_(rnd((m, n), 520 + i).to(dev, torch.bfloat16))
            r.copy_(rnd((m, n), 540 + i).to(dev, torch.bfloat16))
            g.replay()
            st.synchronize()
            want = chain("nt")
            st.synchronize()
            assert torch.equal(_bits(out), _bits(want)), f"replay {i}: {int((_bits(out) != _bits(want)).sum())} of {out.numel()} elements differ"


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
GUARD = 3                                          # guard rows on either side of every output


def _guarded(dev, rows, c, dtype):
    """(whole buffer, the (rows, c) output inside it), NaN pattern everywhere"""
    if dtype == torch.bfloat16:
        w = torch.full((rows + 2 * GUARD, c), PATTERN, dtype=torch.int16, device=dev).view(dtype)
    else:
        w = torch.full((rows + 2 * GUARD, c), PATTERN32, dtype=torch.int32, device=dev).view(dtype)
    return w, w[GUARD:GUARD + rows]


def _ibits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _guards_intact(w, rows):
    pat = PATTERN if w.dtype == torch.bfloat16 else PATTERN32
    g = torch.cat([_ibits(w)[:GUARD], _ibits(w)[GUARD + rows:]])
    return bool((g == pat).all())


# rows 48 (whole wave-iterations at C 768, a workgroup with idle waves at C 64) and 47 (a wave-iteration cut short by the row count)
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [48, 47])
@pytest.mark.parametrize("c", [768, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_layer_norm_stores_cover_every_row_and_no_other(dev, rows, c, dtype):
    ops = _ops()
    L = ops.lib()
    dt = ops.DT[dtype]
    eps = 1e-6
    r_, a_ = (2e-2, 2e-2) if dtype == torch.bfloat16 else (1e-3, 1e-4)
    x = (rnd((rows, c), 601) * 1.3 + 0.2).to(dev, dtype)
    add = rnd((rows, c), 602).to(dev, dtype)
    dy = rnd((rows, c), 603).to(dev, dtype)
    skip = rnd((rows, c), 604).to(dev, dtype)
    gam, bet = (1 + 0.2 * rnd((c,), 605)).to(dev), (0.1 * rnd((c,), 606)).to(dev)
    assert L.vvae_layernorm_supported(c, dt) == 1

    def fwd(addend):
        wy, y = _guarded(dev, rows, c, dtype)
        wx, xs = _guarded(dev, rows, c, dtype) if addend is not None else (None, None)
        mean = torch.empty(rows, device=dev); rstd = torch.empty(rows, device=dev)
        ops.check(L.vvae_layernorm_fwd(_p(x), _p(y), _p(gam), _p(bet), _p(mean), _p(rstd), _p(addend), _p(xs), rows, c, 1, c, 0, eps, dt,
                                       _stream()), "vvae_layernorm_fwd")
        torch.cuda.synchronize()
        assert _guards_intact(wy, rows) and (wx is None or _guards_intact(wx, rows)), "a forward store landed outside the output rows"
        return y, xs, mean, rstd

    def bwd(xin, mean, rstd, dres):
        wd, dx = _guarded(dev, rows, c, dtype)
        part = torch.empty((L.vvae_layernorm_bwd_blocks(rows, c, dt), 2, c), device=dev)
        ops.check(L.vvae_layernorm_bwd(_p(xin), _p(dy), _p(gam), _p(mean), _p(rstd), _p(dres), _p(dx), _p(part), rows, c, 1, c, 0, dt,
                                       _stream()), "vvae_layernorm_bwd")
        torch.cuda.synchronize()
        assert _guards_intact(wd, rows), "a backward store landed outside the output rows"
        return dx

    def formula(xin):
        xr = xin.float().requires_grad_(True)
        mu = xr.mean(-1, keepdim=True)
        var = (xr * xr).mean(-1, keepdim=True) - mu * mu
        return xr, (xr - mu) * torch.rsqrt(var + eps) * gam + bet

    for addend in (None, add):
        y, xs, mean, rstd = fwd(addend)
        y_again, xs_again, _, _ = fwd(addend)
        assert torch.equal(_ibits(y), _ibits(y_again)), "two forward runs differ"
        xin = x
        if addend is not None:
            want_sum = (x.float() + add.float()).to(dtype)
            assert torch.equal(_ibits(xs), _ibits(want_sum)) and torch.equal(_ibits(xs), _ibits(xs_again)), "the fused sum"
            xin = xs.contiguous()
        xr, yr = formula(xin)
        assert bool(torch.isfinite(y).all()), "an element of y still holds the pre-fill"
        assert_close(y, yr, rtol=r_, atol=a_, what="y")
        for dres in (None, skip):
            dx = bwd(xin, mean, rstd, dres)
            dx_again = bwd(xin, mean, rstd, dres)
            assert torch.equal(_ibits(dx), _ibits(dx_again)), "two backward runs differ"
            assert bool(torch.isfinite(dx).all()), "an element of dx still holds the pre-fill"
            (want_dx,) = torch.autograd.grad(yr, xr, dy.float(), retain_graph=True)
            if dres is not None:
                want_dx = want_dx + skip.float()
            assert_close_scaled(dx, want_dx, rel=r_, what="dx")


# ------------------------------------------------------------------------------------------------------------ GroupNorm + SiLU
# (N, T, H, W, C) = (2, 2, 4, 6, C): 48 voxels per sample, one workgroup each; C 16 bf16 / 8 fp32 = two 16-byte channel vectors per voxel
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,c", [(torch.bfloat16, 16), (torch.float32, 8)])
def test_group_norm_silu_stores_cover_a_channel_slice_and_nothing_else(dev, dtype, c):
    """vvae_gn_silu_fwd (write-through stores), and _pool_fwd / _bwd (plain stores, unchanged code: the same property, none of the new
    stores), into the upper channel half of a buffer twice as wide (the concat-elision layout), NaN pattern everywhere first, a guard row
    at either end: every element of the slice is written, no other; two runs are bitwise equal; the values meet the torch formula at
    the tolerances of tests/test_gpu_ops.py::test_group_norm_silu."""
    ops = _ops()
    L = ops.lib()
    dt = ops.DT[dtype]
    n, t, h, w, groups, eps = 2, 2, 4, 6, 4, 1e-6
    s = t * h * w
    ra, rr, rd = (2e-2, 2e-2, 3e-2) if dtype == torch.bfloat16 else (1e-4, 1e-3, 1e-3)
    x = (rnd((n, s, c), 701) * 1.5 + 0.3).to(dev, dtype)
    dy = rnd((n, s, c), 702).to(dev, dtype)
    gam, bet = (1 + 0.2 * rnd((c,), 703)).to(dev), (0.1 * rnd((c,), 704)).to(dev)
    sums = torch.empty((n, groups, 2), dtype=torch.float64, device=dev)
    part = torch.empty(L.vvae_gn_part_floats(n, s, c), device=dev)
    ops.check(L.vvae_gn_stats(_p(x), c, n, s, c, groups, _p(sums), _p(part), dt, _stream()), "vvae_gn_stats")
    pat = PATTERN if dtype == torch.bfloat16 else PATTERN32

    def sliced(rows):
        wide = torch.full((rows + 2, 2 * c), pat, dtype=_ibits(x).dtype, device=dev).view(dtype)
        return wide, wide[1:rows + 1, c:]

    def intact(wide, rows):
        outside = torch.ones_like(wide, dtype=torch.bool)
        outside[1:rows + 1, c:] = False
        return bool((_ibits(wide)[outside] == pat).all())

    def run():
        wy, y = sliced(n * s)
        ops.check(L.vvae_gn_silu_fwd(_p(x), c, _p(y), 2 * c, _p(sums), _p(gam), _p(bet), n, s, c, groups, eps, dt, _stream()), "vvae_gn_silu_fwd")
        wy2, y2 = sliced(n * s)
        wp, pool = sliced(n * s // 4)
        assert L.vvae_gn_silu_pool_supported(h, w, c, groups, c, 2 * c, 2 * c, dt) == 1
        ops.check(L.vvae_gn_silu_pool_fwd(_p(x), c, _p(y2), 2 * c, _p(pool), 2 * c, _p(sums), _p(gam), _p(bet), n, t, h, w, c, groups, eps, dt,
                                          _stream()), "vvae_gn_silu_pool_fwd")
        wd, dx = sliced(n * s)
        csum = torch.empty((n, c, 2), dtype=torch.float64, device=dev)
        dgam, dbet = torch.empty(c, device=dev), torch.empty(c, device=dev)
        ops.check(L.vvae_gn_silu_bwd(_p(x), c, _p(dy), c, _p(dx), 2 * c, _p(sums), _p(gam), _p(bet), _p(csum), _p(part), _p(dgam), _p(dbet),
                                     n, s, c, groups, eps, dt, _stream()), "vvae_gn_silu_bwd")
        torch.cuda.synchronize()
        assert intact(wy, n * s) and intact(wy2, n * s) and intact(wp, n * s // 4) and intact(wd, n * s), "a store landed outside the channel slice"
        return y, y2, pool, dx

    got, again = run(), run()
    for a, b, what in zip(got, again, ("y", "y beside the pool", "pool", "dx")):
        assert torch.equal(_ibits(a), _ibits(b)), f"two runs differ: {what}"
        assert bool(torch.isfinite(a).all()), f"an element of {what} still holds the pre-fill"
    y, y2, pool, dx = got
    assert torch.equal(_ibits(y), _ibits(y2))
    y5 = y.reshape(n, t, h, w, c)
    want_pool = torch.nn.functional.max_pool3d(y5.permute(0, 4, 1, 2, 3).float(), (1, 2, 2)).permute(0, 2, 3, 4, 1).to(dtype)
    assert torch.equal(_ibits(pool.reshape(want_pool.shape)), _ibits(want_pool))
    xr = x.float().requires_grad_(True)
    xg = xr.reshape(n, s, groups, c // groups)
    mu = xg.mean((1, 3), keepdim=True)
    var = (xg * xg).mean((1, 3), keepdim=True) - mu * mu
    z = ((xg - mu) * torch.rsqrt(var + eps)).reshape(n, s, c) * gam + bet
    yr = torch.nn.functional.silu(z)
    (want_dx,) = torch.autograd.grad(yr, xr, dy.float())
    assert_close(y.reshape(n, s, c), yr, rtol=rr, atol=ra, what="y")
    assert_close_scaled(dx.reshape(n, s, c), want_dx, rel=rd, what="dx")


# ------------------------------------------------------------------------------------------------------- spatial attention cores
@pytest.mark.gpu
def test_spatial_attention_stores_cover_their_columns_and_nothing_else(dev):
    """vvae_spatial_attn_fwd / _bwd at their smallest shape (S 32, head_dim 64; 2 sequences x 2 heads = 4 workgroups, each with a
    descriptor over its own rows and columns) into column slices of wider buffers pre-filled with a NaN pattern: ``out`` and all three
    sections of ``dqkv`` are written in full, nothing beside them; two runs are bitwise equal; values against the oracle at the
    tolerances of tests/test_gpu_ops.py::test_spatial_attention_core_bf16."""
    from oracle import layers as OL
    from oracle import nn as O
    ops = _ops()
    L = ops.lib()
    a, s, heads, d, eps, dtype = 2, 32, 2, 64, 1e-6, torch.bfloat16
    hd = heads * d
    qkv = rnd((a, s, 3 * hd), 801).to(dtype)
    go = rnd((a, s, hd), 802).to(dtype)
    qs, ks = 1 + 0.2 * rnd((d,), 803), 1 + 0.2 * rnd((d,), 804)
    cos, sin = OL.rope_tables(d, 256)
    assert L.vvae_spatial_attn_supported(s, d, ops.DT[dtype]) == 1

    xo = qkv.float().requires_grad_(True)
    q, k, v = (z.reshape(a, s, heads, d) for z in torch.chunk(xo, 3, dim=-1))
    qr, kr = OL.rope(O.layer_norm(q, qs, None, dtype), O.layer_norm(k, ks, None, dtype), cos, sin, dtype)
    yo = OL.dot_product_attention(qr, kr, v, None, dtype).reshape(a, s, hd)
    yo.backward(go.float())

    xg, gg = qkv.to(dev), go.to(dev)
    qsg, ksg, cg, sg = qs.to(dev), ks.to(dev), cos.to(dev).contiguous(), sin.to(dev).contiguous()

    def sliced(cols):
        wide = _patterned(dev, a * s + 2, cols + 64)
        return wide, wide[1:a * s + 1, 32:32 + cols]

    def intact(wide, cols):
        outside = torch.ones_like(wide, dtype=torch.bool)
        outside[1:a * s + 1, 32:32 + cols] = False
        return bool((_bits(wide)[outside] == PATTERN).all())

    def run():
        wo, out = sliced(hd)
        lse2 = torch.empty((a * heads, s), device=dev)
        ops.check(L.vvae_spatial_attn_fwd(_p(xg), 3 * hd, _p(out), hd + 64, _p(lse2), _p(qsg), _p(ksg), _p(cg), _p(sg), a, s, heads, d, eps,
                                          ops.DT[dtype], _stream()), "vvae_spatial_attn_fwd")
        wd, dqkv = sliced(3 * hd)
        part = torch.empty((a * heads, 2, d), device=dev)
        ops.check(L.vvae_spatial_attn_bwd(_p(xg), 3 * hd, _p(out), hd + 64, _p(gg), hd, _p(lse2), _p(dqkv), 3 * hd + 64, _p(qsg), _p(ksg), _p(cg),
                                          _p(sg), _p(part), a, s, heads, d, eps, ops.DT[dtype], _stream()), "vvae_spatial_attn_bwd")
        torch.cuda.synchronize()
        assert intact(wo, hd) and intact(wd, 3 * hd), "a store landed outside the output columns"
        return out, dqkv

    (out, dqkv), (out2, dqkv2) = run(), run()
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(dqkv), _bits(dqkv2)), "two runs differ"
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all()), "an output element still holds the pre-fill"
    assert_close(out.reshape(a, s, hd), yo, rtol=3e-2, atol=3e-2, what="out")
    assert_close_scaled(dqkv.reshape(a, s, 3 * hd), xo.grad, rel=5e-2, what="dqkv")
