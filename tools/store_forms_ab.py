"""The kernel families whose 16-byte output stores went write-through (LayerNorm, GroupNorm + SiLU, the spatial attention cores), two builds of
the library side by side in ONE process: every output compared bit for bit first, then GPU microseconds per call from replayed graphs of 20
back-to-back calls (tools/pp_bench_util.tmg), four rounds of parent / this.  gemm_pp has tools/pp_tail_ab.py for the same.

    VVAE_AB_LIB=<the parent build's libvvae_hip.so> python tools/store_forms_ab.py [ln] [gn] [sattn]
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


def load(path):
    l = ctypes.CDLL(os.path.abspath(path))
    for name, (ret, argtypes) in _L.parse_header().items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = ret, argtypes
    return l


if not os.environ.get("VVAE_AB_LIB"):
    sys.exit("usage: VVAE_AB_LIB=<the parent build's libvvae_hip.so> python tools/store_forms_ab.py [ln] [gn] [sattn]")
LIBS = {"parent": load(os.environ["VVAE_AB_LIB"]), "this": load(_L.LIB_PATH)}
p = lambda t: None if t is None else t.data_ptr()
st = lambda: torch.cuda.current_stream().cuda_stream
torch.manual_seed(0)


def layer_norm():
    def case(rows, c, dtype, kind):
        dt = 1 if dtype == torch.bfloat16 else 0
        x = torch.randn(rows, c, device="cuda").to(dtype); add = torch.randn(rows, c, device="cuda").to(dtype)
        dy = torch.randn(rows, c, device="cuda").to(dtype)
        gam = torch.randn(c, device="cuda"); bet = torch.randn(c, device="cuda")
        y = torch.empty_like(x); xs = torch.empty_like(x); dx = torch.empty_like(x)
        mean = torch.empty(rows, device="cuda"); rstd = torch.empty(rows, device="cuda")
        nblk = LIBS["this"].vvae_layernorm_bwd_blocks(rows, c, dt)
        part = torch.empty(nblk, 2, c, device="cuda")
        LIBS["parent"].vvae_layernorm_fwd(p(x), p(y), p(gam), p(bet), p(mean), p(rstd), None, None, rows, c, 1, c, 0, 1e-6, dt, st())
        def run(l):
            if kind == "fwd": rc = l.vvae_layernorm_fwd(p(x), p(y), p(gam), p(bet), p(mean), p(rstd), None, None, rows, c, 1, c, 0, 1e-6, dt, st())
            elif kind == "addfwd": rc = l.vvae_layernorm_fwd(p(x), p(y), p(gam), p(bet), p(mean), p(rstd), p(add), p(xs), rows, c, 1, c, 0, 1e-6, dt, st())
            elif kind == "bwd": rc = l.vvae_layernorm_bwd(p(x), p(dy), p(gam), p(mean), p(rstd), None, p(dx), p(part), rows, c, 1, c, 0, dt, st())
            else: rc = l.vvae_layernorm_bwd(p(x), p(dy), p(gam), p(mean), p(rstd), p(add), p(dx), p(part), rows, c, 1, c, 0, dt, st())
            assert rc == 0, rc
        return run, (y, xs, dx, part)
    print("LayerNorm: bitwise, this build against the parent:")
    for rows, c, dtype in [(16384, 768, torch.bfloat16), (48, 768, torch.bfloat16), (47, 64, torch.bfloat16), (1000, 512, torch.float32), (131072, 64, torch.bfloat16)]:
        for kind in ("fwd", "addfwd", "bwd", "bwdskip"):
            run, outs = case(rows, c, dtype, kind)
            got = []
            for l in LIBS.values():
                for o in outs: o.zero_()
                run(l); torch.cuda.synchronize()
                got.append([o.clone() for o in outs])
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*got))
            print(f"  rows {rows} C {c} {str(dtype)[6:]} {kind}: {'identical' if same else 'DIFFERENT'}", flush=True)
            assert same
    print("us per launch (graph of 20), rounds of parent / this:")
    for rows, c, kind in [(16384, 768, "fwd"), (16384, 768, "addfwd"), (16384, 768, "bwd"), (16384, 768, "bwdskip"), (16384 * 12, 64, "fwd")]:
        run, _ = case(rows, c, torch.bfloat16, kind)
        row = []
        for _ in range(4):
            for name, l in LIBS.items():
                row.append(f"{name} {tmg(lambda: run(l)):6.2f}")
        print(f"  rows {rows} C {c} {kind}: " + " | ".join(row), flush=True)


def group_norm_silu():
    def case(n, t, h, w, c, g, kind, dtype=torch.bfloat16):
        dt = 1 if dtype == torch.bfloat16 else 0
        s = t * h * w
        x = torch.randn(n, s, c, device="cuda").to(dtype); dy = torch.randn(n, s, c, device="cuda").to(dtype)
        gam = torch.randn(c, device="cuda"); bet = torch.randn(c, device="cuda")
        y = torch.empty(n, s, 2 * c, device="cuda", dtype=dtype)[..., c:]; pool = torch.empty(n, s // 4, c, device="cuda", dtype=dtype); dx = torch.empty_like(x)
        sums = torch.empty(n, g, 2, dtype=torch.float64, device="cuda"); csum = torch.empty(n, c, 2, dtype=torch.float64, device="cuda")
        L0 = LIBS["parent"]
        part = torch.empty(L0.vvae_gn_part_floats(n, s, c), device="cuda"); dg = torch.empty(c, device="cuda"); db = torch.empty(c, device="cuda")
        assert L0.vvae_gn_stats(p(x), c, n, s, c, g, p(sums), p(part), dt, st()) == 0
        def run(l):
            if kind == "fwd": rc = l.vvae_gn_silu_fwd(p(x), c, p(y), 2 * c, p(sums), p(gam), p(bet), n, s, c, g, 1e-6, dt, st())
            elif kind == "pool": rc = l.vvae_gn_silu_pool_fwd(p(x), c, p(y), 2 * c, p(pool), c, p(sums), p(gam), p(bet), n, t, h, w, c, g, 1e-6, dt, st())
            else: rc = l.vvae_gn_silu_bwd(p(x), c, p(dy), c, p(dx), c, p(sums), p(gam), p(bet), p(csum), p(part), p(dg), p(db), n, s, c, g, 1e-6, dt, st())
            assert rc == 0, rc
        return run, (y, pool, dx)
    print("GroupNorm + SiLU: bitwise, this build against the parent:")
    for shape in [(4, 16, 64, 64, 32, 8), (2, 2, 4, 6, 16, 4), (1, 3, 10, 14, 64, 8), (4, 16, 128, 128, 16, 8)]:
        for kind in ("fwd", "pool", "bwd"):
            for dtype in (torch.bfloat16, torch.float32):
                run, outs = case(*shape, kind, dtype)
                got = []
                for l in LIBS.values():
                    for o in outs: o.zero_()
                    run(l); torch.cuda.synchronize()
                    got.append([o.clone() for o in outs])
                same = all(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) for a, b in zip(*got))
                print(f"  {shape} {kind} {str(dtype)[6:]}: {'identical' if same else 'DIFFERENT'}", flush=True)
                assert same
    print("us per call (graph of 20; bwd = reduce + finalize + apply), rounds of parent / this:")
    for shape in [(4, 16, 64, 64, 32, 8), (4, 16, 128, 128, 16, 8), (4, 16, 32, 32, 64, 8)]:
        for kind in ("fwd", "pool", "bwd"):
            run, _ = case(*shape, kind)
            row = []
            for _ in range(4):
                for name, l in LIBS.items():
                    row.append(f"{name} {tmg(lambda: run(l)):6.2f}")
            print(f"  {shape} {kind}: " + " | ".join(row), flush=True)


def spatial_attention():
    from oracle import layers as OL
    cos, sin = OL.rope_tables(64, 256)
    cos, sin = cos.cuda().contiguous(), sin.cuda().contiguous()
    def case(a, s, heads, kind):
        d = 64; hd = heads * d
        qkv = torch.randn(a * s, 3 * hd, device="cuda").bfloat16(); go = torch.randn(a * s, hd, device="cuda").bfloat16()
        qs = torch.randn(d, device="cuda"); ks = torch.randn(d, device="cuda")
        out = torch.empty(a * s, hd, device="cuda", dtype=torch.bfloat16); dqkv = torch.empty_like(qkv)
        lse2 = torch.empty(a * heads, s, device="cuda"); part = torch.empty(a * heads, 2, d, device="cuda")
        fwd = lambda l: l.vvae_spatial_attn_fwd(p(qkv), 3 * hd, p(out), hd, p(lse2), p(qs), p(ks), p(cos), p(sin), a, s, heads, d, 1e-6, 1, st())
        bwd = lambda l: l.vvae_spatial_attn_bwd(p(qkv), 3 * hd, p(out), hd, p(go), hd, p(lse2), p(dqkv), 3 * hd, p(qs), p(ks), p(cos), p(sin), p(part), a, s, heads, d, 1e-6, 1, st())
        assert fwd(LIBS["parent"]) == 0
        def run(l):
            rc = fwd(l) if kind == "fwd" else bwd(l)
            assert rc == 0, rc
        return run, (out, dqkv, part)
    print("spatial attention: bitwise, this build against the parent:")
    for a, s, heads in [(64, 256, 8), (2, 32, 2), (3, 160, 3)]:
        for kind in ("fwd", "bwd"):
            run, outs = case(a, s, heads, kind)
            got = []
            for l in LIBS.values():
                for o in outs[1:]: o.zero_()
                run(l); torch.cuda.synchronize()
                got.append([o.clone() for o in outs])
            same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(*got))
            print(f"  A{a} S{s} H{heads} {kind}: {'identical' if same else 'DIFFERENT'}", flush=True)
            assert same
    print("us per launch (graph of 20), rounds of parent / this:")
    for kind in ("fwd", "bwd"):
        run, _ = case(64, 256, 8, kind)
        row = []
        for _ in range(4):
            for name, l in LIBS.items():
                row.append(f"{name} {tmg(lambda: run(l)):6.2f}")
        print(f"  A64 S256 H8 {kind}: " + " | ".join(row), flush=True)


FAMILIES = {"ln": layer_norm, "gn": group_norm_silu, "sattn": spatial_attention}
for name in (sys.argv[1:] or list(FAMILIES)):
    FAMILIES[name]()
