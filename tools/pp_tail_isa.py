#!/usr/bin/env python3
"""Price the epilogue tails of gemm_pp from the ISA, without a GPU: compile gemm_pp.hip to gfx950 assembly and print, per instantiation of the
256 x 192 kernel, the registers, the private segment, the instruction mix and a run-length trace of every region of the code that holds stores
(a mid-launch or a final epilogue): how many vector / transcendental instructions sit between which stores, fragment reads and barriers.

    python tools/pp_tail_isa.py [--trace] [extra hipcc flags]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "video_vae_amd", "csrc", "gemm_pp.hip")
MAKEFILE = os.path.join(ROOT, "video_vae_amd", "csrc", "Makefile")
EPI = {0: "EPI_NONE", 1: "EPI_RES", 2: "EPI_SILU", 3: "EPI_MUL_DSILU"}


def flags():
    """The library's own compile flags (CXXFLAGS of csrc/Makefile, its ARCH filled in), so that what is priced is what is shipped."""
    mk = open(MAKEFILE).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    cxx = re.search(r"^CXXFLAGS\s*=\s*(.+)$", mk, flags=re.M).group(1)
    return cxx.replace("$(ARCH)", arch).split()


def assembly(extra=()):
    """gfx950 assembly of gemm_pp.hip; a failing compile raises with hipcc's messages."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "pp.s")
        r = subprocess.run(["hipcc", *flags(), "--cuda-device-only", "-S", *extra, SRC, "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {SRC} (status {r.returncode}):\n{r.stderr[-4000:]}")
        return open(out).read()


def kind(op):
    op = re.sub(r"_(e32|e64|sdwa|dpp)$", "", op)
    if op.startswith("v_mfma"): return "mfma"
    if op in ("v_exp_f32", "v_rcp_f32", "v_log_f32", "v_rsq_f32", "v_sqrt_f32"): return "trans"
    if op.startswith("global_store"): return "store"
    if op.startswith("global_load_lds"): return "dma"
    if op.startswith("global_load"): return "gload"
    if op.startswith("ds_read") or op.startswith("ds_load"): return "dsr_b128" if "b128" in op else "dsr"
    if op.startswith("ds_write") or op.startswith("ds_store"): return "dsw"
    if op.startswith("scratch_"): return "scratch"
    if op == "s_barrier": return "BARRIER"
    if op == "s_waitcnt": return "wait"
    if op.startswith("v_"): return "valu"
    if op.startswith("s_cbranch") or op == "s_branch": return "branch"
    return "salu"


def functions(asm):
    """-> {mangled name: [(label or None, op)]} for the gemm_pp kernels, and {name: metadata dict}."""
    fns, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(_ZN2pp14gemm_pp_kernel\w+):", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            cur.append((m.group(1), None))
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\b", line)
        if m and not line.lstrip().startswith("."):
            cur.append((None, m.group(1)))
    meta = {}
    for m in re.finditer(r"\.name:\s+(_ZN2pp14gemm_pp_kernel\w+)\n(.*?)\.wavefront_size", asm, flags=re.S):
        body = m.group(2)
        meta[m.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", body).group(1)) for k in
                            ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_count")}
    return fns, meta


def blocks(ins):
    out, cur = [], ["entry", []]
    for label, op in ins:
        if label:
            out.append(cur)
            cur = [label, []]
        else:
            cur[1].append(op)
    out.append(cur)
    return [b for b in out if b[1]]


def rle(ops):
    out = []
    for op in ops:
        k = kind(op)
        if k in ("wait", "salu"):
            continue
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return " ".join(f"{k}x{n}" if n > 1 else k for k, n in out)


def main():
    args = sys.argv[1:]
    trace = "--trace" in args
    extra = [a for a in args if a != "--trace"]
    fns, meta = functions(assembly(extra))
    for name in sorted(fns):
        m = re.search(r"CfgILi256ELi(\d+)EEELi(\d)ELi(\d)E", name)
        if not m or m.group(1) != "192" or m.group(3) != "0":
            continue
        epi = int(m.group(2))
        md = meta.get(name, {})
        print(f"== Cfg<256,192> {EPI[epi]}: vgpr {md.get('vgpr_count')}, spilled {md.get('vgpr_spill_count')}, "
              f"private segment {md.get('private_segment_fixed_size')} B")
        for label, ops in blocks(fns[name]):
            c = {}
            for op in ops:
                c[kind(op)] = c.get(kind(op), 0) + 1
            if not c.get("store"):
                continue
            ex = sum(op.startswith("v_exp_f32") for op in ops)
            rc = sum(op.startswith("v_rcp_f32") for op in ops)
            print(f"   block {label}: {len(ops)} instructions, stores {c.get('store', 0)}, tail loads {c.get('gload', 0)}, valu {c.get('valu', 0)}, "
                  f"v_exp {ex}, v_rcp {rc}, v_cvt_pk_bf16 {sum(op.startswith('v_cvt_pk_bf16') for op in ops)}, ds_write {c.get('dsw', 0)}, ds_read_b128 {c.get('dsr_b128', 0)}, dma {c.get('dma', 0)}, "
                  f"mfma {c.get('mfma', 0)}, barriers {c.get('BARRIER', 0)}, waits {c.get('wait', 0)}")
            if trace:
                print("      " + rle(ops))


if __name__ == "__main__":
    main()
