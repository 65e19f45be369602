"""gemm_pp's fused SiLU and SiLU' tails (csrc/gemm_pp.hip: EPI_SILU, EPI_MUL_DSILU), bit for bit, in eager mode and inside a replayed graph, at the
trunk's MLP shape (M 16 384, N 1536, K 768: two tiles per workgroup, so a mid-launch and a final epilogue) and at one small shape.

What a tail is documented to equal: the plain product (EPI_NONE, + bias) rounded to bf16, then the elementwise op on the ROUNDED value.
  * the saved pre-activation of EPI_SILU IS that rounded product: compared bitwise with the EPI_NONE launch;
  * the activations are compared bitwise with torch's op on the rounded product of the EPI_NONE launch WHEREVER the first kernel form,
    gemm_nt.hip, meets that comparison, and bitwise with gemm_nt.hip under the same epilogue everywhere.  gemm_nt.hip evaluates the same
    expression (x * v_rcp_f32(1 + v_exp_f32(-x log2 e)), rounded once) straight from its accumulators, and tests/test_gpu_ops.py holds gemm_pp to
    it bit for bit, so "gemm_nt differs from torch's op in this element" is exactly "gemm_pp did before the epilogue was reworked": the
    hardware's exp and reciprocal are approximations, torch's are not the same ones, and where the two fp32 values straddle a bf16 rounding
    boundary the last bit differs.  The test therefore asserts that gemm_pp differs from torch's op in the SAME elements as gemm_nt and in no
    other (all of them, if gemm_nt matches torch everywhere), and prints how many those are.
A host-only test scans the ISA of the two instantiations: no private segment (scratch), no spilled registers.
"""
import os
import re
import shutil
import sys

import pytest
import torch

from util import rnd

SHAPES = [(16384, 1536, 768), (512, 384, 128)]


def _ops():
    from video_vae_amd import ops
    return ops


def _inputs(dev, m, n, k):
    a = rnd((m, k), 401).to(dev, torch.bfloat16)
    b = (rnd((n, k), 402) / k ** 0.5).to(dev, torch.bfloat16)
    bias = rnd((n,), 403).to(dev)
    h = rnd((m, n), 404, 2.0).to(dev, torch.bfloat16)           # a saved pre-activation for the backward tail
    return a, b, bias, h


def _run(ops, form, a, b, bias, h):
    plain = ops.gemm_nt(a, b, bias, form=form)
    plain_nobias = ops.gemm_nt(a, b, form=form)
    act, pre = ops.gemm_nt(a, b, bias, None, ops.EPI_SILU, form=form)
    dx = ops.gemm_nt(a, b, None, h, ops.EPI_MUL_DSILU, form=form)
    return plain, plain_nobias, act, pre, dx


def _ulps(x, y):
    """distance in bf16 steps between two bf16 tensors (sign-magnitude order)"""
    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(x) - key(y)).abs()


def _check(ops, got, want, plain_for_ref, h, what):
    plain, plain_nobias, act, pre, dx = got
    w_plain, w_plain_nobias, w_act, w_pre, w_dx = want
    assert torch.equal(pre, plain), f"{what}: the saved pre-activation is the rounded plain product"
    assert torch.equal(plain, w_plain) and torch.equal(plain_nobias, w_plain_nobias), f"{what}: plain product against gemm_nt"
    assert torch.equal(pre, w_pre), f"{what}: pre-activation against gemm_nt"
    assert torch.equal(act, w_act), f"{what}: silu tail against gemm_nt, {int((act != w_act).sum())} differ"
    assert torch.equal(dx, w_dx), f"{what}: silu' tail against gemm_nt, {int((dx != w_dx).sum())} differ"
    # torch's op on the rounded product: bitwise wherever the first kernel form matches it, i.e. wherever gemm_pp matched it before
    t_act = torch.nn.functional.silu(plain.float()).to(torch.bfloat16)
    hf = h.float()
    s = torch.sigmoid(hf)
    t_dx = (plain_nobias.float() * (s * (1 + hf * (1 - s)))).to(torch.bfloat16)
    for name, g_, w_, t_ in (("silu", act, w_act, t_act), ("silu'", dx, w_dx, t_dx)):
        off, off_nt = g_ != t_, w_ != t_
        print(f"{what}: {name} against torch on the rounded product: gemm_pp {int(off.sum())}, gemm_nt {int(off_nt.sum())} of {g_.numel()} differ "
              f"(at most {int(_ulps(g_, t_).max())} bf16 steps)")
        assert torch.equal(off, off_nt), f"{what}: {name} differs from torch's op where gemm_nt does not: {int((off & ~off_nt).sum())} elements"
        assert torch.equal(g_[~off_nt], t_[~off_nt])


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_tails_eager(dev, m, n, k):
    ops = _ops()
    a, b, bias, h = _inputs(dev, m, n, k)
    assert ops.lib().vvae_gemm_pp_supported(m, n, k, k, k, n) == 1 and ops.gemm_nt_supported(a, b)
    want = _run(ops, "nt", a, b, bias, h)
    got = _run(ops, "pp", a, b, bias, h)
    _check(ops, got, want, got[0], h, f"eager {m}x{n}x{k}")


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_tails_in_a_replayed_graph(dev, m, n, k):
    ops = _ops()
    a, b, bias, h = _inputs(dev, m, n, k)
    want = _run(ops, "nt", a, b, bias, h)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        _run(ops, "pp", a, b, bias, h)                         # warm: function attributes are set outside the capture
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            got = _run(ops, "pp", a, b, bias, h)
        for t in got:
            t.fill_(3.0)                                       # a replay has to write every element again
        g.replay()
        g.replay()
        st.synchronize()
    torch.cuda.synchronize()
    _check(ops, got, want, got[0], h, f"graph {m}x{n}x{k}")


def test_tail_kernels_have_no_scratch_and_no_spills():
    """Host only: gemm_pp.hip compiled to gfx950 assembly; the SiLU and SiLU' instantiations of both tiles keep everything in registers."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import pp_tail_isa
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not found")
    asm = pp_tail_isa.assembly()                               # a compile failure fails the test, with hipcc's messages
    _, meta = pp_tail_isa.functions(asm)
    seen = 0
    for name, md in meta.items():
        m = re.search(r"CfgILi256ELi(\d+)EEELi(\d)ELi0E", name)
        if not m or m.group(2) not in ("2", "3"):
            continue
        seen += 1
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["vgpr_count"] <= 256, (name, md)             # two waves per SIMD
    assert seen == 4, sorted(meta)
