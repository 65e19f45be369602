"""The T = 16 matrix-core temporal attention cores (csrc/attn_temporal_mfma.hip), two or more builds of the library side by side in ONE
process: o, lse, dqkv and the scale-gradient partial rows compared bit for bit against the parent build first, then GPU microseconds per
launch from replayed graphs of 20 back-to-back launches (tools/pp_bench_util.tmg), four rounds over the builds, at the benchmark's shape
(A = 4 x 256 sequences, 8 heads, the strided (b, t, hw, c) layout), masked and unmasked.

    VVAE_AB_LIB=<the parent build's libvvae_hip.so> [VVAE_AB_VARIANTS=name=path,name=path] python tools/tattn_ab.py [bits] [time]

VVAE_AB_VARIANTS names further builds of this tree (other compile-time choices of the same kernels) to put beside "parent" and "this".
"""
import ctypes
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import video_vae_amd._lib as _L
from pp_bench_util import tmg
from oracle import layers as OL

T, D = 16, 64


def load(path):
    l = ctypes.CDLL(os.path.abspath(path))
    for name, (ret, argtypes) in _L.parse_header().items():
        if hasattr(l, name):                      # an older build lacks the hooks added since
            fn = getattr(l, name)
            fn.restype, fn.argtypes = ret, argtypes
    return l


if not os.environ.get("VVAE_AB_LIB"):
    sys.exit(__doc__)
LIBS = {"parent": load(os.environ["VVAE_AB_LIB"])}
for item in filter(None, os.environ.get("VVAE_AB_VARIANTS", "").split(",")):
    name, path = item.split("=", 1)
    LIBS[name] = load(path)
LIBS["this"] = load(_L.LIB_PATH)
p = lambda t: None if t is None else t.data_ptr()
st = lambda: torch.cuda.current_stream().cuda_stream
torch.manual_seed(0)
cos, sin = OL.rope_tables(D, 64)
cos = cos.to(torch.bfloat16).float().cuda().contiguous()
sin = sin.to(torch.bfloat16).float().cuda().contiguous()


def case(a, heads, inner, mask_div):
    """mask_div 0: no mask.  -> (fwd(lib), bwd(lib), outputs)"""
    hd = heads * D
    tokens = a * T
    qkv = torch.randn(tokens, 3 * hd, device="cuda").bfloat16()
    go = torch.randn(tokens, hd, device="cuda").bfloat16()
    qs = 1 + 0.2 * torch.randn(D, device="cuda"); ks = 1 + 0.2 * torch.randn(D, device="cuda")
    mask = None
    if mask_div:
        nm = (a + mask_div - 1) // mask_div
        lens = torch.tensor([max(1, T - (i * 5) % T) for i in range(nm)])
        mask = (torch.arange(T)[None, :] < lens[:, None]).to(torch.uint8).cuda()
    out = torch.empty(tokens, hd, device="cuda", dtype=torch.bfloat16); dqkv = torch.empty_like(qkv)
    lse = torch.empty(a * heads, T, device="cuda")
    nblk = LIBS["parent"].vvae_temporal_attn_fast_blocks(a, T, heads, D, 1)
    part = torch.empty(nblk, 2 * D, device="cuda")
    md = max(mask_div, 1)

    def fwd(l):
        rc = l.vvae_temporal_attn_fwd_fast(p(qkv), 3 * hd, p(out), hd, p(lse), p(qs), p(ks), p(cos), p(sin), p(mask), md, inner, a, T, heads, D,
                                           1e-6, 1, st())
        assert rc == 0, rc

    def bwd(l):
        rc = l.vvae_temporal_attn_bwd_fast(p(qkv), 3 * hd, p(out), hd, p(go), hd, p(lse), p(dqkv), 3 * hd, p(qs), p(ks), p(cos), p(sin), p(mask),
                                           md, inner, p(part), a, T, heads, D, 1e-6, 1, st())
        assert rc == 0, rc
    return fwd, bwd, (out, lse, dqkv, part)


def bits():
    print("bitwise against the parent build: o, lse, dqkv, part rows")
    for a, heads, inner in [(5, 3, 1), (12, 8, 4), (600, 8, 1), (1024, 8, 256)]:
        for mask_div in (0, 1, 2 * inner):
            fwd, bwd, outs = case(a, heads, inner, mask_div)
            ref = None
            for name, l in LIBS.items():
                for o in outs: o.zero_()
                fwd(l); bwd(l); torch.cuda.synchronize()
                got = [o.clone() for o in outs]
                if ref is None:
                    ref = got
                    continue
                same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(ref, got))
                print(f"  A{a} H{heads} inner{inner} mask_div{mask_div} {name}: {'identical' if same else 'DIFFERENT'}", flush=True)
                assert same


def time_():
    print("us per launch (graph of 20) at A1024 H8 inner256, rounds over " + " / ".join(LIBS))
    for mask_div in (0, 256):
        fwd, bwd, _ = case(1024, 8, 256, mask_div)
        fwd(LIBS["parent"])
        for kind, run in (("fwd", fwd), ("bwd", bwd)):
            row = []
            for _ in range(4):
                row.append(" ".join(f"{name} {tmg(lambda: run(l)):6.2f}" for name, l in LIBS.items()))
            print(f"  {kind} {'masked' if mask_div else 'unmasked'}: " + " | ".join(row), flush=True)


PARTS = {"bits": bits, "time": time_}
for name in (sys.argv[1:] or list(PARTS)):
    PARTS[name]()
