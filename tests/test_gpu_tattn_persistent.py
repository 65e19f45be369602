"""The T = 16 matrix-core temporal attention cores (csrc/attn_temporal_mfma.hip) as persistent kernels: a launch holds no more workgroups
than stay resident, every wave walks its items in a loop with the RoPE tables and scale vectors loaded once, the next item's rows in
flight and its LDS images handed over from item to item.  What an item computes must not depend on which wave gets it, in which round:

  * schedule independence: the grid capped at 1, at 3 and not at all (vvae_temporal_attn_mfma_config) gives the same bits of o, lse, dqkv,
    the partial rows and the folded scale gradients;
  * the VALU kernels of attn_temporal_fast.hip (vvae_temporal_attn_mfma_enable(0)), an independent implementation, on the same inputs,
    at the tolerances tests/test_gpu_ops.py::test_temporal_attention_matrix_core_kernels holds this pair to (out: rtol = atol = 2e-2,
    dqkv: 3e-2 of its scale; the scale gradients at the 5e-2 of their scale that test asks of either implementation);
  * two runs on the same buffers inside one captured graph give the same bits (the hand-over of the LDS images between loop rounds).

Shapes, bf16, T = 16, D = 64: (A 5, 3 heads): 15 items, a partial last group, groups that straddle sequences; (A 12, 8 heads, inner 4):
the strided (b, t, hw, c) layout; (A 600, 8 heads): 4 800 items in 1 200 groups, more than any resident grid, so the default iterates
too.  Each without a mask, with one mask row per sequence and with a mask row shared by several sequences, every row a different tail.
"""
import pytest
import torch

from oracle import layers as OL
from util import assert_close, assert_close_scaled, rnd

pytestmark = pytest.mark.gpu

T, D = 16, 64
SHAPES = [(5, 3, 1), (12, 8, 4), (600, 8, 1)]
MASKS = ["none", "div1", "shared"]
CAPS = (1, 3, 0)


def _ops():
    from video_vae_amd import ops
    return ops


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_CASES = {}


def _case(dev, a, heads, inner, mask_kind):
    """Inputs of one case, made once."""
    key = (a, heads, inner, mask_kind)
    if key not in _CASES:
        hd = heads * D
        seed = 900 + 10 * SHAPES.index((a, heads, inner)) + MASKS.index(mask_kind)
        c = {"a": a, "heads": heads, "inner": inner, "hd": hd}
        c["qkv"] = rnd((a * T, 3 * hd), seed).to(dev, torch.bfloat16)
        c["go"] = rnd((a * T, hd), seed + 100).to(dev, torch.bfloat16)
        c["qs"] = (1 + 0.2 * rnd((D,), seed + 200)).to(dev)
        c["ks"] = (1 + 0.2 * rnd((D,), seed + 300)).to(dev)
        cos, sin = OL.rope_tables(D, 64)
        c["cos"] = cos.to(torch.bfloat16).float().to(dev).contiguous()
        c["sin"] = sin.to(torch.bfloat16).float().to(dev).contiguous()
        c["mask_div"] = {"none": 1, "div1": 1, "shared": 2 if inner == 1 else inner}[mask_kind]
        c["mask"] = None
        if mask_kind != "none":
            nm = (a + c["mask_div"] - 1) // c["mask_div"]
            lens = torch.tensor([max(1, T - (i * 5 + 3) % T) for i in range(nm)])
            c["mask"] = (torch.arange(T)[None, :] < lens[:, None]).to(torch.uint8).to(dev)
        _CASES[key] = c
    return _CASES[key]


def _buffers(c, dev):
    ops = _ops()
    a, heads, hd = c["a"], c["heads"], c["hd"]
    nblk = ops.lib().vvae_temporal_attn_fast_blocks(a, T, heads, D, 1)
    return (torch.zeros((a * T, hd), dtype=torch.bfloat16, device=dev), torch.zeros((a * heads, T), device=dev),
            torch.zeros((a * T, 3 * hd), dtype=torch.bfloat16, device=dev), torch.zeros((nblk, 2 * D), device=dev))


def _launch(c, bufs):
    ops = _ops()
    L = ops.lib()
    out, lse, dqkv, part = bufs
    a, heads, hd = c["a"], c["heads"], c["hd"]
    ops.check(L.vvae_temporal_attn_fwd_fast(_p(c["qkv"]), 3 * hd, _p(out), hd, _p(lse), _p(c["qs"]), _p(c["ks"]), _p(c["cos"]), _p(c["sin"]),
                                            _p(c["mask"]), c["mask_div"], c["inner"], a, T, heads, D, 1e-6, 1, _stream()), "fwd")
    ops.check(L.vvae_temporal_attn_bwd_fast(_p(c["qkv"]), 3 * hd, _p(out), hd, _p(c["go"]), hd, _p(lse), _p(dqkv), 3 * hd, _p(c["qs"]),
                                            _p(c["ks"]), _p(c["cos"]), _p(c["sin"]), _p(c["mask"]), c["mask_div"], c["inner"], _p(part), a, T,
                                            heads, D, 1e-6, 1, _stream()), "bwd")


def _run(c, dev, cap=0, mfma=True):
    """-> (o, lse, dqkv, part, folded dq_scale, folded dk_scale)"""
    ops = _ops()
    L = ops.lib()
    try:
        L.vvae_temporal_attn_mfma_enable(1 if mfma else 0)
        assert L.vvae_temporal_attn_mfma_config(cap) == 0
        bufs = _buffers(c, dev)
        _launch(c, bufs)
        dqs, dks = ops.fold_partials(bufs[3], None, None, D)
        torch.cuda.synchronize()
        return bufs + (dqs, dks)
    finally:
        L.vvae_temporal_attn_mfma_config(0)
        L.vvae_temporal_attn_mfma_enable(1)


_DEFAULT = {}


def _default(c, dev):
    """The default-grid result of a case, computed once and left unchanged."""
    key = id(c)
    if key not in _DEFAULT:
        _DEFAULT[key] = _run(c, dev)
    return _DEFAULT[key]


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


NAMES = ("o", "lse", "dqkv", "part", "dq_scale", "dk_scale")


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("a,heads,inner", SHAPES)
def test_results_do_not_depend_on_the_grid(dev, a, heads, inner, mask_kind):
    c = _case(dev, a, heads, inner, mask_kind)
    assert _ops().lib().vvae_temporal_attn_fast_blocks(a, T, heads, D, 1) == (a * heads + 3) // 4
    ref = _default(c, dev)
    assert bool(torch.isfinite(ref[0].float()).all()) and bool(torch.isfinite(ref[2].float()).all())
    for cap in CAPS:
        got = _run(c, dev, cap=cap)
        for name, x, y in zip(NAMES, got, ref):
            assert _same_bits(x, y), f"grid cap {cap}: {name} differs from the default grid's in {int((x != y).sum())} of {x.numel()} elements"


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("a,heads,inner", SHAPES)
def test_against_the_valu_kernels(dev, a, heads, inner, mask_kind):
    c = _case(dev, a, heads, inner, mask_kind)
    new = _default(c, dev)
    old = _run(c, dev, mfma=False)
    assert_close(new[0], old[0], rtol=2e-2, atol=2e-2, what="out, matrix-core vs VALU")
    assert_close_scaled(new[2], old[2], rel=3e-2, what="dqkv, matrix-core vs VALU")
    assert_close_scaled(new[4], old[4], rel=5e-2, what="dq_scale, matrix-core vs VALU")
    assert_close_scaled(new[5], old[5], rel=5e-2, what="dk_scale, matrix-core vs VALU")


@pytest.mark.parametrize("cap", [3, 0])
def test_two_runs_in_one_captured_graph_agree(dev, cap):
    c = _case(dev, 600, 8, 1, "shared")
    L = _ops().lib()
    st = torch.cuda.Stream()
    try:
        assert L.vvae_temporal_attn_mfma_config(cap) == 0
        with torch.cuda.stream(st):
            bufs = _buffers(c, dev)
            _launch(c, bufs)                                   # warm: the resident-grid query runs outside the capture
            st.synchronize()
            for b in bufs:
                b.zero_()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                _launch(c, bufs)
                first = [b.clone() for b in bufs]
                _launch(c, bufs)
            g.replay()
            st.synchronize()
    finally:
        L.vvae_temporal_attn_mfma_config(0)
    ref = _default(c, dev)
    for name, x, y, z in zip(NAMES, first, bufs, ref):
        assert _same_bits(x, y), f"{name}: the second run in the graph differs from the first"
        assert _same_bits(x, z), f"{name}: the run in the graph differs from the eager one"
