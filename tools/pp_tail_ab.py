"""gemm_pp per launch, two builds of the library alternately in ONE process: the four epilogues at M 16 384, N1536 K768 (and the residual shape
N768 K1536), GPU microseconds per call from replayed graphs of 20 back-to-back calls, ``--rounds`` times A / B / A / B; the outputs of the two
builds are compared bit for bit first (with and without a bias, plus two small shapes).  With ``--ablation-lib`` (a -DPP_ABLATION build of the
working tree) the SiLU / SiLU' launches are also timed with their activation arithmetic replaced by a move (bit 16): what the arithmetic costs.

    VVAE_AB_LIB=<the other build's libvvae_hip.so[,a third build's]> python tools/pp_tail_ab.py [--rounds 3] [--ablation-lib path]
"""
import argparse
import ctypes
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import video_vae_amd._lib as _L
from pp_bench_util import tmg

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--ablation-lib", default=None)
args = ap.parse_args()


def load(path):
    l = ctypes.CDLL(os.path.abspath(path))
    for name, (ret, argtypes) in _L.parse_header().items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = ret, argtypes
    return l


if not os.environ.get("VVAE_AB_LIB"):
    sys.exit("usage: VVAE_AB_LIB=<other build's libvvae_hip.so[,a third build's]> python tools/pp_tail_ab.py [--rounds 3] [--ablation-lib path]")
LIBS = {os.path.basename(q).replace("libvvae_", "").replace(".so", ""): load(q) for q in os.environ["VVAE_AB_LIB"].split(",")}       # several: a,b
LIBS["this"] = load(_L.LIB_PATH)
M = 16384
torch.manual_seed(0)
p = lambda t: None if t is None else t.data_ptr()


def case(m, n, k, epi, with_bias=True):
    a = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
    b = (torch.randn(n, k, device="cuda") / k ** 0.5).to(torch.bfloat16)
    bias = torch.randn(n, device="cuda") if with_bias and epi != 3 else None
    res = torch.randn(m, n, device="cuda", dtype=torch.bfloat16) if epi in (1, 3) else None
    c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
    c2 = torch.empty(m, n, device="cuda", dtype=torch.bfloat16) if epi == 2 else None

    def run(l):
        st = torch.cuda.current_stream().cuda_stream
        rc = l.vvae_gemm_pp_bf16(p(a), k, p(b), k, p(c), n, p(bias), p(res), n if res is not None else 0, p(c2), n, epi, m, n, k, st)
        assert rc == 0, rc
    return run, c, c2


print("bitwise, this build against the other:")
for (m, n, k) in [(M, 1536, 768), (M, 768, 1536), (512, 384, 128), (256, 128, 192), (1024, 1536, 768)]:
    for epi in range(4):
        for wb in (True, False):
            run, c, c2 = case(m, n, k, epi, wb)
            outs = []
            for l in LIBS.values():
                c.fill_(7.0)
                if c2 is not None:
                    c2.fill_(7.0)
                run(l)
                torch.cuda.synchronize()
                outs.append((c.clone(), None if c2 is None else c2.clone()))
            same = all(torch.equal(outs[0][0].view(torch.int16), o[0].view(torch.int16)) and (
                c2 is None or torch.equal(outs[0][1].view(torch.int16), o[1].view(torch.int16))) for o in outs[1:])
            print(f"  M{m} N{n} K{k} epi{epi} bias={'yes' if wb and epi != 3 else 'no'}: {'identical' if same else 'DIFFERENT'}", flush=True)
            assert same

print("us per launch (graph of 20), rounds of other / this:")
for (n, k, epi) in [(1536, 768, 0), (1536, 768, 2), (1536, 768, 3), (768, 1536, 1), (768, 768, 0)]:
    run, c, c2 = case(M, n, k, epi)
    row = []
    for _ in range(args.rounds):
        for name, l in LIBS.items():
            row.append(f"{name} {tmg(lambda: run(l)):6.2f}")
    print(f"  N{n} K{k} epi{epi}: " + " | ".join(row), flush=True)

if args.ablation_lib:
    la = load(args.ablation_lib)
    print("ablation build of this tree: full tail / tail arithmetic replaced by a move (bit 16), us per launch:")
    for epi in (0, 2, 3):
        run, c, c2 = case(M, 1536, 768, epi)
        row = []
        for _ in range(args.rounds):
            for bits in (0, 16):
                la.vvae_gemm_pp_ablate(bits)
                row.append(f"{'move' if bits else 'full'} {tmg(lambda: run(la)):6.2f}")
        la.vvae_gemm_pp_ablate(0)
        print(f"  N1536 K768 epi{epi}: " + " | ".join(row), flush=True)
