"""The kernels that only move data, element for element: max-pool (1,2,2) forward and backward, un-patchify + channel pad, the grouped
weight pads, the grouped transposes, and the SiLU stream.

None of them has arithmetic that can be wrong.  What can be wrong is an index, a pitch, the vector or scalar choice, a grid cap or an
entry lookup.  So every result here is defined bit for bit (the SiLU values excepted) and every bound is zero:

  * Max-pool, vvae_maxpool_1x2x2_fwd / _bwd (pool_convt.hip).  The forward is a selection: y is one of the four inputs of its window.
    The backward is dx = dskip (or 0) + (first strict maximum of the window, in the order (0,0), (0,1), (1,0), (1,1) ? dpool : 0): a
    selection and ONE addition.  The reference is that sentence in index arithmetic on the CPU (pool_ref); for every small case the
    builder also holds it against torch autograd through oracle.nn.max_pool_1x2x2, in fp32 and fp64.
      Family I, integers: x in {-2 ... 2} (five values in a window of four: every tie pattern occurs), some zeros planted as -0.0, dpool
        and dskip in {-8 ... 8}: every sum is an integer of the dtype (util.assert_representable), so the bound is zero.
        util.assert_exact counts the two zeros as one.
      Family R, one rounded addition: Gaussian x, dpool and dskip, already numbers of the dtype.  The expected value is
        (dskip.float() + dpool.float()).to(dtype): one fp32 addition and one round-to-nearest-even, which is what the kernel's store
        does.  Zero tolerance in both dtypes.  (bf16 Gaussians do tie now and then; the reference resolves a tie as the kernel must.)
    NaN: the forward folds the window with fmaxf, which drops a NaN operand (a window of NaN and numbers yields the largest number); the
    backward's `>` is false against a NaN, so a NaN never wins over an earlier element.  This is stated, not tested.
    The misaligned cases make one operand a slice that starts at channel 4 of a 24-channel buffer: 8-byte aligned in bf16.  In fp32 that
    slice is 16-byte aligned and still vectorises, so the fp32 rows start at channel 2 (8-byte aligned again).
    The cases at and past the grid cap check forward and both backward forms in one test each, so the CPU reference is built once; it is
    moved to the device and compared there.

  * Un-patchify + pad, vvae_unpatch_pad_fwd / _bwd (unpatch.hip), the grouped pads, vvae_pad_last2_grouped (pad_channels.hip) and the
    grouped transposes, vvae_transpose_grouped_bf16 (loss_optim.hip), are byte movers: the inputs are integer bit patterns (a counter
    times an odd multiplier, NaN, infinity and denormal encodings planted in front), the references are reshape / permute / F.pad /
    slice / .t() on the CPU, and the comparison is on the integers.  The benchmark's own un-patchify geometry (16 x 16 patches of 16,
    12 -> 16 channels) is the one case with h = w; it and (3, 4, 3, 8, 12, 16) fill their last workgroup exactly (2048 / 1536 and 36 / 27
    workgroups), every other total is ragged.

  * SiLU stream, vvae_silu_bf16: the values are held at the bar test_silu_stream_kernel uses (fp64 SiLU rounded to bf16, rtol 2^-7,
    atol 1e-6).  Exact on top of that: the input is one Gaussian block tiled over the buffer, and equal inputs must give equal bits
    wherever they lie (the unrolled trip and the tail trips are the same arithmetic).

Every output buffer is allocated with guards in front and behind (and between packed destinations) and filled, guards and the complement
of every channel slice included, with a NaN bit pattern that no input holds.  After the launch the WHOLE buffer is compared: what the
kernel does not own must be unchanged bit for bit ("guards"), what it owns must hold no poison ("unwritten") and must equal the reference
("values").  No element is exempt anywhere.  A refusal must raise VvaeError and leave the poisoned destination untouched.

Every case asserts the regime it means to be in -- vector width per operand, workgroups, trips of the grid-stride loop for the first and
the last workgroup -- from Python mirrors of vvae_pool_blocks, vvae_pool_vec and vvae_silu_blocks, which are held against the library (the
launchers call the same three functions).  Retuning a cap fails these assertions instead of silently shrinking the coverage.

Each builder validates its case on the CPU before a GPU result is looked at.  tests/test_host.py runs the builders without a GPU
(HOST_CHECKS: regimes, representability, and a CPU restatement of each kernel's own index arithmetic passing the very assertions the GPU
results meet) and feeds the assertions a restatement with one defect each (DEFECT_CHECKS): every one must raise in the assertion named.
"""
import ctypes
import functools
import math
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import nn as O
from util import assert_close, assert_exact, assert_representable, ints, rnd

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
INT = {BF16: torch.int16, F32: torch.int32}
POISON = {torch.int16: 0x7FA5, torch.int32: 0x7FA5A5A5}          # a NaN in bf16 and in fp32: never equal to anything, never an input
PAD_NAN = -73                                                     # 0xFFB7, what the pad channels of the un-patchify cotangent hold
GUARD = 64                                                        # elements; keeps every part 16-byte aligned in either width
DT = {F32: 0, BF16: 1}
WINDOW = ((0, 0), (0, 1), (1, 0), (1, 1))


class _Case(types.SimpleNamespace):
    pass


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31 - 1000)


def _lib():
    from video_vae_amd._lib import lib
    return lib()


def _ops():
    from video_vae_amd import ops
    return ops


def _raises(fn, match):
    with pytest.raises(AssertionError, match=match):
        fn()


# =========================================================================================== the three queries, mirrored
POOL_CAP, SILU_CAP = 8192, 4096          # pool_convt.hip: vvae_pool_blocks; loss_optim.hip: vvae_silu_blocks


def pool_blocks(items):
    return min(items // 256 + 1, POOL_CAP)


def pool_vec(ptr, ld, c, dtype):
    v = 8 if dtype == BF16 else 4
    return v if c % v == 0 and ld % v == 0 and ptr % 16 == 0 else 1


def silu_blocks(nvec):
    return min((nvec + 1023) // 1024, SILU_CAP)


def stride_trips(items, blocks, b):
    """Trips of the grid-stride loop `for (it = b * 256 + tid; it < items; it += blocks * 256)` that reach at least lane 0 of workgroup b."""
    first = b * 256
    return 0 if first >= items else -(-(items - first) // (blocks * 256))


def silu_trips(nvec, blocks, i):
    """(unrolled trips, tail trips) of global thread i of silu_bf16_kernel."""
    s, u, t = blocks * 256, 0, 0
    while i + 3 * s < nvec:
        u, i = u + 1, i + 4 * s
    while i < nvec:
        t, i = t + 1, i + s
    return u, t


def _mirrors_match_the_library():
    """Both sides of every boundary of the three queries."""
    lb = _lib()
    for items in (0, 1, 255, 256, 257, 256 * 8190 + 255, 256 * 8191 - 1, 256 * 8191, 256 * 8191 + 1, 256 * 8192, 2102784, 1 << 33):
        assert lb.vvae_pool_blocks(items) == pool_blocks(items), items
    assert pool_blocks(256 * 8191 - 1) == 8191 and pool_blocks(256 * 8191) == 8192 == pool_blocks(1 << 33) == POOL_CAP
    for nvec in (0, 1, 1023, 1024, 1025, 1024 * 4095, 1024 * 4095 + 1, 1024 * 4096, 1024 * 4096 + 1, 6 * 4096 * 256 + 1000, 1 << 33):
        assert lb.vvae_silu_blocks(nvec) == silu_blocks(nvec), nvec
    assert silu_blocks(1024 * 4095) == 4095 and silu_blocks(1024 * 4095 + 1) == 4096 == silu_blocks(1 << 33) == SILU_CAP
    base = 1 << 20
    for dtype in (BF16, F32):
        v = 8 if dtype == BF16 else 4
        for ptr in (base, base + 2, base + 4, base + 8, base + 16, base + 32):
            for ld in (v, v - 1, v + 1, 2 * v, 3 * v, 24, 20, 7):
                for c in (v, 2 * v, v // 2, v + 1, 3 * v, 1, 6, 12, 16):
                    want = pool_vec(ptr, ld, c, dtype)
                    assert lb.vvae_pool_vec(ctypes.c_void_p(ptr), ld, c, DT[dtype]) == want, (dtype, ptr, ld, c, want)
        assert pool_vec(base, 2 * v, v, dtype) == v and pool_vec(base + 8, 2 * v, v, dtype) == 1 and pool_vec(base, 2 * v + 1, v, dtype) == 1
    assert lb.vvae_pool_vec(ctypes.c_void_p(base), 16, 16, 7) == 1                     # an unknown dtype never vectorises


# =========================================================================================== poisoned buffers
def _fresh(n, itype, device):
    return torch.full((n,), POISON[itype], dtype=itype, device=device)


def _first(bad):
    return int(bad.reshape(-1).nonzero()[0])


class Slab:
    """guard | rows x width | guard, all poison; ``view`` is the channel slice [off, off + c) of the rows, in ``dtype``."""

    def __init__(self, lead, c, width, off, dtype, device, values=None):
        assert 0 <= off and off + c <= width
        self.lead, self.c, self.width, self.off, self.dtype = tuple(lead), c, width, off, dtype
        self.rows = math.prod(self.lead)
        self.base = GUARD + off                                   # flat index of channel 0 of row 0
        self.flat = _fresh(2 * GUARD + self.rows * width, INT[dtype], device).view(dtype)
        self.view = self._slice(self.flat)
        if values is not None:
            self.view.copy_(values.to(dtype))

    def _slice(self, flat):
        return flat[GUARD:GUARD + self.rows * self.width].view(*self.lead, self.width)[..., self.off:self.off + self.c]

    def to(self, device):
        s = Slab.__new__(Slab)
        s.__dict__.update(self.__dict__)
        s.flat = self.flat.to(device)
        s.view = s._slice(s.flat)
        return s

    def check(self, want, what):
        """The whole buffer: unchanged outside the slice, no poison inside, the slice equal to ``want`` (the two zeros count as one)."""
        it = INT[self.dtype]
        rest = self.flat.view(it).clone()
        self._slice(rest).fill_(POISON[it])
        bad = rest != POISON[it]
        nbad = int(bad.sum())
        assert nbad == 0, (f"{what}: guards: {nbad} elements outside the slice changed; first at flat index {_first(bad) if nbad else -1} "
                           f"(guard {GUARD}, pitch {self.width}, slice [{self.off}, {self.off + self.c}))")
        left = self.view.view(it) == POISON[it]
        nleft = int(left.sum())
        assert nleft == 0, (f"{what}: unwritten: {nleft}/{left.numel()} owned elements still hold the poison; first at "
                            f"{tuple(left.nonzero()[0].tolist()) if nleft else ()}")
        assert_exact(self.view, want, f"{what}: values")

    def untouched(self, what):
        bad = self.flat.view(INT[self.dtype]) != POISON[INT[self.dtype]]
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of a refused call's destination were written"


class Packed:
    """guard | part 0 | guard | part 1 | ... | guard of integer bit patterns, all poison; every part starts on a multiple of GUARD."""

    def __init__(self, sizes, itype, device, values=None, shift=0):
        self.sizes, self.itype, self.offs = list(sizes), itype, []
        o = GUARD + shift
        for s in self.sizes:
            self.offs.append(o)
            o += -(-s // GUARD) * GUARD + GUARD
        self.flat = _fresh(o, itype, device)
        if values is not None:
            for i, v in enumerate(values):
                self.part(i).copy_(v.reshape(-1))

    def part(self, i, flat=None):
        flat = self.flat if flat is None else flat
        return flat[self.offs[i]:self.offs[i] + self.sizes[i]]

    def to(self, device):
        s = Packed.__new__(Packed)
        s.__dict__.update(self.__dict__)
        s.flat = self.flat.to(device)
        return s

    def check(self, wants, what):
        """The whole buffer against poison + ``wants`` (integer tensors, one per part), bitwise."""
        p = POISON[self.itype]
        exp = _fresh(self.flat.numel(), self.itype, "cpu")
        own = torch.zeros(self.flat.numel(), dtype=torch.bool)
        for i, w in enumerate(wants):
            assert w.dtype == self.itype and w.numel() == self.sizes[i], (what, i, w.dtype, w.numel(), self.sizes[i])
            assert not bool((w == p).any()), f"{what}: part {i}: the reference holds the poison pattern"
            self.part(i, exp).copy_(w.reshape(-1))
            self.part(i, own).fill_(True)
        exp, own = exp.to(self.flat.device), own.to(self.flat.device)
        bad = (self.flat != exp) & ~own
        nbad = int(bad.sum())
        assert nbad == 0, f"{what}: guards: {nbad} elements outside the destinations changed; first at flat index {_first(bad) if nbad else -1}"
        left = (self.flat == p) & own
        nleft = int(left.sum())
        assert nleft == 0, f"{what}: unwritten: {nleft}/{int(own.sum())} owned elements still hold the poison; {self._where(left) if nleft else ''}"
        bad = self.flat != exp
        nbad = int(bad.sum())
        assert nbad == 0, f"{what}: values: {nbad}/{int(own.sum())} owned elements differ; {self._where(bad, exp) if nbad else ''}"

    def _where(self, bad, exp=None):
        j = _first(bad)
        i = max(k for k, o in enumerate(self.offs) if o <= j)
        s = f"first at part {i}, index {j - self.offs[i]} of {self.sizes[i]}"
        return s if exp is None else s + f": got {int(self.flat[j]):#x} want {int(exp[j]):#x}"

    def untouched(self, what):
        bad = self.flat != POISON[self.itype]
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of a refused call's destination were written"


def patterns(n, seed, itype=torch.int16):
    """n integer bit patterns: a counter times an odd multiplier, with NaN, infinity, denormal and signed-zero encodings of the float
    format of that width planted in front; never the poison, never PAD_NAN."""
    if itype == torch.int16:
        v = (torch.arange(n, dtype=torch.int64) * 40503 + seed * 7919 + 12345) & 0xFFFF
        special = [0x7FC0, 0xFFA6, 0x0001, 0x807F, 0x7F80, 0xFF80, 0x8000, 0x0000, 0x7F81]
        avoid, top = [POISON[itype], PAD_NAN & 0xFFFF], 1 << 16
    else:
        v = (torch.arange(n, dtype=torch.int64) * 2654435761 + seed * 7919 + 12345) & 0xFFFFFFFF
        special = [0x7FC00000, 0xFFA5A5A6, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7F800001]
        avoid, top = [POISON[itype]], 1 << 32
    if n >= 2 * len(special):
        v[:len(special)] = torch.tensor(special, dtype=torch.int64)
    for a in avoid:
        v = torch.where(v == a, v ^ 2, v)
    return torch.where(v >= top // 2, v - top, v).to(itype)


# =========================================================================================== max-pool (1,2,2)
POOL_OPS = {"fwd": ("x", "y"), "bwd0": ("x", "dpool", "dx"), "bwd1": ("x", "dpool", "dskip", "dx")}
POOL_MODES = ("fwd", "bwd0", "bwd1")


def pool_layout(name, c, dtype):
    """operand -> (pitch, first channel) of the buffer its channel slice lives in."""
    if name == "contig":
        return {op: (c, 0) for op in ("x", "y", "dpool", "dskip", "dx")}
    if name == "pitched":                  # five pitches; x is the upper half of a 2C joint buffer, as unet.py holds a level's skip
        return {"x": (2 * c, c), "y": (3 * c, c), "dpool": (4 * c, 2 * c), "dskip": (5 * c, 3 * c), "dx": (6 * c, c)}
    if name == "odd":                      # five odd pitches, slices that start anywhere
        return {"x": (c + 1, 1), "y": (c + 3, 2), "dpool": (c + 5, 3), "dskip": (c + 7, 5), "dx": (c + 9, 7)}
    assert name.startswith("mis-") and c == 16
    lay = {op: (c, 0) for op in ("x", "y", "dpool", "dskip", "dx")}
    lay[name[4:]] = (24, 4 if dtype == BF16 else 2)              # 8-byte aligned in either dtype
    return lay


def pool_ref(x, dpool, dskip, dtype):
    """-> (y, dx without dskip, dx with dskip) in ``dtype``, then y and dx without dskip as computed: plain index arithmetic, the first
    strict maximum wins."""
    xs = [x[:, :, a::2, b::2] for a, b in WINDOW]
    best, arg = xs[0], torch.zeros(xs[0].shape, dtype=torch.int8)
    for k in (1, 2, 3):
        better = xs[k] > best
        best, arg = torch.where(better, xs[k], best), torch.where(better, k, arg)
    dx0, dx1 = torch.zeros_like(x), dskip.clone()
    for k, (a, b) in enumerate(WINDOW):
        hit = torch.where(arg == k, dpool, 0.0)
        dx0[:, :, a::2, b::2] = hit
        dx1[:, :, a::2, b::2] += hit                              # one fp32 addition; the cast below is the one rounding
    return best.to(dtype), dx0.to(dtype), dx1.to(dtype), best, dx0


@functools.lru_cache(maxsize=2)
def pool_case(family, geo, dtype, layout="contig", vw=None, blocks=None, trips=None):
    """``vw``: the per-operand vector width the case claims (8 / 4 / 1); ``blocks``, ``trips``: claimed workgroups and (first, last) trips of
    the vector-or-scalar launch every mode of the case makes, None = one sweep below the cap."""
    n, t, h, w, c = geo
    k = _Case(family=family, geo=geo, dtype=dtype, layout=layout, lay=pool_layout(layout, c, dtype), vw=vw, blocks=blocks, trips=trips,
              mis=layout[4:] if layout.startswith("mis-") else None, what=f"pool {family} {geo} {str(dtype)[6:]} {layout}")
    sx, sp = (n, t, h, w, c), (n, t, h // 2, w // 2, c)
    sd = _seed("pool", family, geo, str(dtype), layout)
    if family == "I":
        x = ints(sx, sd, -2, 2)
        neg = torch.rand(sx, generator=torch.Generator().manual_seed(sd + 3)) < 0.5
        x = torch.where((x == 0) & neg, -0.0, x)                  # -0.0 / +0.0 pairs: equal, so the first of them wins a tie
        dpool, dskip = ints(sp, sd + 1, -8, 8), ints(sx, sd + 2, -8, 8)
    else:
        x, dpool, dskip = (rnd(s, sd + i).to(dtype).float() for i, s in enumerate((sx, sp, sx)))
    k.x, k.dpool, k.dskip = x, dpool, dskip
    k.y, k.dx0, k.dx1, y_raw, dx0_raw = pool_ref(x, dpool, dskip, dtype)
    # ---- validity, before any GPU result
    for name, v in (("x", x), ("dpool", dpool), ("dskip", dskip)):
        assert bool((v.to(dtype).float() == v).all()), f"{k.what}: {name} is not a number of the dtype"
    assert torch.equal(k.y.float(), y_raw) and torch.equal(k.dx0.float(), dx0_raw), f"{k.what}: a selection must survive the dtype"
    if family == "I":
        assert_representable(k.dx1.float(), dtype, 16)
        assert bool((k.dx1.float() == dskip + dx0_raw).all())
        if x.numel() >= 64:
            wins = torch.stack([x[:, :, a::2, b::2] == y_raw for a, b in WINDOW]).sum(0)
            assert int((wins > 1).sum()) > 0 and bool((torch.signbit(x) & (x == 0)).any()), f"{k.what}: no ties / no -0.0 in the case"
    else:
        want = (dskip.float() + dx0_raw.float()).to(dtype)
        assert torch.equal(k.dx1, want)
    if x.numel() <= 1 << 16:                                      # the tie rule is the oracle's, in fp32 and fp64
        for fd in (torch.float32, torch.float64):
            xa = x.detach().to(fd).clone().requires_grad_(True)
            ya = O.max_pool_1x2x2(xa)
            (ga,) = torch.autograd.grad(ya, xa, dpool.to(fd))
            assert bool((ya.detach() == y_raw.to(fd)).all()) and bool((ga == dx0_raw.to(fd)).all()), f"{k.what}: oracle autograd, {fd}"
    return k


def pool_bufs(k, device):
    """The three input slabs (poison in the complement of each slice: a read outside the slice meets a NaN)."""
    n, t, h, w, c = k.geo
    lead = {"x": (n, t, h, w), "dskip": (n, t, h, w), "dx": (n, t, h, w), "y": (n, t, h // 2, w // 2), "dpool": (n, t, h // 2, w // 2)}
    k.lead = lead
    host = {op: Slab(lead[op], c, *k.lay[op], k.dtype, "cpu", getattr(k, op)) for op in ("x", "dpool", "dskip")}
    return {op: s.to(device) for op, s in host.items()} if str(device) != "cpu" else host


def pool_out(k, mode, device):
    op = "y" if mode == "fwd" else "dx"
    return op, Slab(k.lead[op], k.geo[4], *k.lay[op], k.dtype, device)


def pool_regime(k, bufs, mode, lib=None):
    """-> launch vector width.  Asserts the per-operand widths, the workgroups and the trips the case claims."""
    n, t, h, w, c = k.geo
    widths = {}
    for op in POOL_OPS[mode]:
        s = bufs[op]
        ptr = s.view.data_ptr()
        if s.flat.device.type == "cpu":                           # the host allocator's alignment is not the device's: an aligned base + the offset
            ptr = (1 << 20) + (ptr - s.flat.data_ptr())
        widths[op] = pool_vec(ptr, s.width, c, k.dtype)
        if lib is not None:
            assert lib.vvae_pool_vec(ctypes.c_void_p(ptr), s.width, c, DT[k.dtype]) == widths[op], (k.what, mode, op)
    claim = {op: (1 if op == k.mis else k.vw) for op in POOL_OPS[mode]}
    assert widths == claim, f"{k.what}: {mode}: vector width per operand {widths}, the case claims {claim}"
    full = 8 if k.dtype == BF16 else 4
    vec = full if all(v == full for v in widths.values()) else 1
    assert vec == (1 if k.mis in POOL_OPS[mode] else k.vw), (k.what, mode, vec)
    items = n * t * (h // 2) * (w // 2) * (c // vec)
    blocks = pool_blocks(items)
    if lib is not None:
        assert lib.vvae_pool_blocks(items) == blocks
    got = (blocks, stride_trips(items, blocks, 0), stride_trips(items, blocks, blocks - 1))
    if k.blocks is None:
        assert blocks < POOL_CAP and got[1] == 1 and got[2] in (0, 1) and items <= blocks * 256, f"{k.what}: {mode}: not one sweep: {got}"
    else:
        assert got == (k.blocks,) + tuple(k.trips), f"{k.what}: {mode}: (workgroups, first trips, last trips) = {got}, the case claims {(k.blocks,) + tuple(k.trips)}"
    return vec


def cpu_pool(k, bufs, mode, vec, defect=None):
    """The kernels' own index arithmetic on the flat buffers (item -> channel vector, window, plane; pointer + voxel * pitch + channel),
    in torch on the CPU."""
    n, t, h, w, c = k.geo
    cv, ho_, wo_ = c // vec, h // 2, w // 2
    items = n * t * ho_ * wo_ * cv
    it = torch.arange(items)
    if defect == "second trip skipped":
        it = it[it < pool_blocks(items) * 256]
    c0, q = (it % cv) * vec, it // cv
    wo, q = q % wo_, q // wo_
    ho, p = q % ho_, q // ho_
    vi = (p * h + 2 * ho) * w + 2 * wo
    vs = (vi, vi + 1, vi + w, vi + w + 1)
    vp = (p * ho_ + ho) * wo_ + wo
    lane = torch.arange(vec)

    def at(s, vox, ld=None):
        return (s.base + vox[:, None] * (ld or s.width) + c0[:, None] + lane[None, :]) % s.flat.numel()

    xin = [bufs["x"].flat[at(bufs["x"], v)].float() for v in vs]
    if mode == "fwd":
        y = bufs["y"]
        y.flat[at(y, vp)] = torch.maximum(torch.maximum(xin[0], xin[1]), torch.maximum(xin[2], xin[3])).to(k.dtype)
        if defect == "writes a channel outside the slice":
            y.flat[y.base + c] = 0.0
        return
    g = bufs["dpool"].flat[at(bufs["dpool"], vp)].float()
    best, arg = xin[0], torch.zeros(xin[0].shape, dtype=torch.int8)
    for j in (1, 2, 3):
        better = xin[j] >= best if defect == "last tie wins" else xin[j] > best
        best, arg = torch.where(better, xin[j], best), torch.where(better, j, arg)
    dx, ds = bufs["dx"], bufs["dskip"]
    for j in range(4):
        out = torch.zeros_like(g)
        if mode == "bwd1" and defect != "dskip dropped":
            out = ds.flat[at(ds, vs[j], dx.width if defect == "dskip read with dx's pitch" else None)].float()
        hit = xin[j] == best if defect == "every tied maximum receives" else arg == j
        dx.flat[at(dx, vs[j])] = (out + torch.where(hit, g, 0.0)).to(k.dtype)


def check_pool(k, out, mode):
    out.check(k.y if mode == "fwd" else k.dx0 if mode == "bwd0" else k.dx1, f"{k.what}: {mode}")


def pool_modes(k):
    return [m for m in POOL_MODES if k.mis is None or k.mis in POOL_OPS[m]]


def _pool_host(make, defect=None, mode=None):
    k = make()
    bufs = pool_bufs(k, "cpu")
    for m in ([mode] if mode else pool_modes(k)):
        op, out = pool_out(k, m, "cpu")
        bufs[op] = out
        vec = pool_regime(k, bufs, m, _lib())
        cpu_pool(k, bufs, m, vec, defect)
        check_pool(k, out, m)


SMALL_POOL = [((2, 3, 8, 6, 16), BF16, 8), ((2, 3, 8, 6, 16), F32, 4), ((2, 3, 8, 6, 24), BF16, 8), ((2, 3, 8, 6, 24), F32, 4),
              ((2, 3, 8, 6, 12), BF16, 1), ((2, 3, 8, 6, 12), F32, 4), ((2, 3, 8, 6, 6), BF16, 1), ((2, 3, 8, 6, 6), F32, 1),
              ((2, 3, 8, 6, 1), BF16, 1), ((2, 3, 8, 6, 1), F32, 1), ((1, 2, 2, 2, 8), BF16, 8), ((1, 2, 2, 2, 8), F32, 4),
              ((3, 1, 2, 10, 16), BF16, 8), ((3, 1, 2, 10, 16), F32, 4), ((1, 1, 10, 2, 16), BF16, 8), ((1, 1, 10, 2, 16), F32, 4)]
PITCHED_POOL = [((2, 3, 8, 6, 16), BF16, "pitched", 8), ((2, 3, 8, 6, 16), F32, "pitched", 4),
                ((2, 3, 8, 6, 6), BF16, "odd", 1), ((2, 3, 8, 6, 6), F32, "odd", 1)]
MIS_POOL = [(op, dtype) for dtype in (BF16, F32) for op in ("x", "y", "dpool", "dskip", "dx")]
# (geometry, dtype, claimed operand width, workgroups, (first, last) trips).  Items: 64*128*128*2 = 2 097 152 = 8192 * 256, one full sweep;
# 592*592*6 = 2 102 784 = one sweep + 5 632 (22 workgroups); 1024*1026*2 = 512*1026*4 = 2 101 248 = one sweep + 4 096 (16 workgroups).
CAP_POOL = [((64, 1, 256, 256, 16), BF16, 8, 8192, (1, 1)), ((1, 1, 1184, 1184, 6), BF16, 1, 8192, (2, 1)), ((1, 1, 1184, 1184, 6), F32, 1, 8192, (2, 1)),
            ((1, 1, 2048, 2052, 16), BF16, 8, 8192, (2, 1)), ((1, 1, 1024, 2052, 16), F32, 4, 8192, (2, 1))]


def _pool_makers():
    out = []
    for fam in ("I", "R"):
        for geo, dtype, vw in SMALL_POOL:
            out.append((f"pool-{fam}-{'x'.join(map(str, geo))}-{str(dtype)[6:]}", functools.partial(pool_case, fam, geo, dtype, "contig", vw)))
        for geo, dtype, lay, vw in PITCHED_POOL:
            out.append((f"pool-{fam}-{lay}-{geo[4]}-{str(dtype)[6:]}", functools.partial(pool_case, fam, geo, dtype, lay, vw)))
        for op, dtype in MIS_POOL:
            out.append((f"pool-{fam}-mis-{op}-{str(dtype)[6:]}",
                        functools.partial(pool_case, fam, (2, 3, 8, 6, 16), dtype, "mis-" + op, 8 if dtype == BF16 else 4)))
        for geo, dtype, vw, blocks, trips in CAP_POOL:
            out.append((f"pool-{fam}-cap-{'x'.join(map(str, geo))}-{str(dtype)[6:]}",
                        functools.partial(pool_case, fam, geo, dtype, "contig", vw, blocks, trips)))
    return out


def _second_sweep_is_ragged():
    for geo, dtype, vw, blocks, trips in CAP_POOL[1:]:
        n, t, h, w, c = geo
        items = n * t * (h // 2) * (w // 2) * (c // vw)
        rest = items - POOL_CAP * 256
        assert 0 < rest < POOL_CAP * 256 and rest == {6: 5632, 16: 4096}[c] and -(-rest // 256) == {6: 22, 16: 16}[c], (geo, rest)
    n, t, h, w, c = CAP_POOL[0][0]
    assert n * t * (h // 2) * (w // 2) * (c // 8) == POOL_CAP * 256 == 2097152


def _pool_defects():
    pitched = functools.partial(pool_case, "I", (2, 3, 8, 6, 16), BF16, "pitched", 8)
    past = functools.partial(pool_case, "I", (1, 1, 1184, 1184, 6), F32, "contig", 1, 8192, (2, 1))
    rows = [("last tie wins", pitched, "bwd1", r"bwd1: values: \d+/\d+ "), ("every tied maximum receives", pitched, "bwd0", r"bwd0: values: \d+/\d+ "),
            ("second trip skipped", past, "fwd", r"fwd: unwritten: 5632/"), ("second trip skipped", past, "bwd1", r"bwd1: unwritten: 22528/"),
            ("dskip dropped", pitched, "bwd1", r"bwd1: values: \d+/\d+ "), ("dskip read with dx's pitch", pitched, "bwd1", r"bwd1: values: \d+/\d+ "),
            ("writes a channel outside the slice", pitched, "fwd", r"fwd: guards: 1 elements")]
    return [(f"pool-{d.replace(' ', '-')}-{m}", functools.partial(_raises, functools.partial(_pool_host, make, d, m), match)) for d, make, m, match in rows]


# =========================================================================================== un-patchify + pad
UNPATCH = [(1, 1, 1, 1, 4, 4), (2, 3, 5, 2, 12, 16), (3, 4, 3, 8, 12, 16), (1, 2, 7, 4, 4, 16), (5, 1, 6, 3, 8, 12), (1, 3, 2, 2, 20, 32),
           (2, 16, 16, 16, 12, 16)]              # (frames, h, w, p, cu, c); the last is the benchmark decoder's (256 / 16, patch 16, 3 * 4 -> 16) at 2 frames
BENCH_UNPATCH = UNPATCH[-1]
UNPATCH_BLOCK_EXACT = (UNPATCH[2], BENCH_UNPATCH)          # 36 / 27 and 2048 / 1536 full workgroups; every other total is ragged


def unpatch_fwd_ref(x, geo):
    f, h, w, p, cu, c = geo
    return F.pad(x.view(f, h, w, p, p, cu).permute(0, 1, 3, 2, 4, 5).reshape(f, h * p, w * p, cu), (0, c - cu))


def unpatch_bwd_ref(g, geo):
    f, h, w, p, cu, c = geo
    return g[..., :cu].reshape(f, h, p, w, p, cu).permute(0, 1, 3, 2, 4, 5).reshape(f, h * w, p * p * cu)


@functools.lru_cache(maxsize=2)
def unpatch_case(geo):
    f, h, w, p, cu, c = geo
    k = _Case(geo=geo, what=f"unpatch {geo}")
    k.x = patterns(f * h * w * p * p * cu, _seed("up", geo)).view(f, h * w, p * p * cu)
    k.y = unpatch_fwd_ref(k.x, geo).contiguous()
    k.g = patterns(f * h * p * w * p * c, _seed("upg", geo)).view(f, h * p, w * p, c).clone()
    k.g[..., cu:] = PAD_NAN
    k.gx = unpatch_bwd_ref(k.g, geo).contiguous()
    # ---- validity
    assert cu % 4 == 0 and c % 4 == 0 and c >= cu
    assert torch.equal(unpatch_bwd_ref(k.y, geo), k.x) and bool((k.y[..., cu:] == 0).all()), f"{k.what}: the two references are not transposes"
    assert torch.equal(k.gx.reshape(-1).sort().values, k.g[..., :cu].reshape(-1).sort().values) and not bool((k.gx == PAD_NAN).any())
    k.pieces = (k.y.numel() // 4, k.gx.numel() // 4)
    k.blocks = tuple(-(-v // 256) for v in k.pieces)
    assert geo == BENCH_UNPATCH or h != w or min(h, w) == 1, f"{k.what}: h == w"
    if geo in UNPATCH_BLOCK_EXACT:
        assert not any(v % 256 for v in k.pieces) and k.pieces == {BENCH_UNPATCH: (524288, 393216)}.get(geo, (9216, 6912))
    else:
        assert all(v % 256 for v in k.pieces), f"{k.what}: a block-exact total"
    return k


def cpu_unpatch(k, src, dst, backward, defect=None):
    """unpatch_pad_fwd_kernel / _bwd_kernel in 8-byte pieces on the flat buffers."""
    f, h, w, p, cu, c = k.geo
    cu4, c4 = cu // 4, c // 4
    s4, d4 = src.part(0).view(-1, 4), dst.part(0).view(-1, 4)
    n = f * h * p * w * p
    per = cu4 if backward else c4
    i = torch.arange(n * per)
    if defect == "last workgroup skipped":
        i = i[i < (-(-i.numel() // 256) - 1) * 256]
    q, v = i % per, i // per
    xx, v = v % (w * p), v // (w * p)
    yy, fr = v % (h * p), v // (h * p)
    hi, p1, wi, p2 = yy // p, yy % p, xx // p, xx % p
    if defect == "p1 and p2 swapped":
        p1, p2 = p2, p1
    cell = (fr * w + wi) * h + hi if defect == "h and w swapped in the source offset" else (fr * h + hi) * w + wi
    piece = cell * (p * p * cu4) + (p1 * p + p2) * cu4
    if backward:
        d4[piece + q] = s4[((i // cu4) * (cu4 if defect == "g indexed with the unpadded pitch" else c4) + q) % s4.shape[0]]
        return
    real = q < cu4
    if defect != "pad channels unwritten":
        d4[i[~real]] = 0
    d4[i[real]] = s4[(piece + q)[real]]


def _unpatch_bufs(k, backward, device):
    src = Packed([(k.g if backward else k.x).numel()], torch.int16, "cpu", [k.g if backward else k.x])
    dst = Packed([(k.gx if backward else k.y).numel()], torch.int16, device)
    return (src.to(device) if str(device) != "cpu" else src), dst


def _unpatch_host(geo, defect=None, only=None):
    k = unpatch_case(geo)
    for backward in ((False, True) if only is None else (only,)):
        src, dst = _unpatch_bufs(k, backward, "cpu")
        cpu_unpatch(k, src, dst, backward, defect)
        dst.check([k.gx if backward else k.y], f"{k.what}: {'bwd' if backward else 'fwd'}")


def _unpatch_defects():
    geo = (2, 3, 5, 2, 12, 16)
    rows = [("p1 and p2 swapped", False, r"fwd: values: "), ("p1 and p2 swapped", True, r"bwd: values: "),
            ("h and w swapped in the source offset", False, r"fwd: values: "), ("h and w swapped in the source offset", True, r"bwd: values: "),
            ("pad channels unwritten", False, r"fwd: unwritten: 480/1920 "), ("g indexed with the unpadded pitch", True, r"bwd: values: "),
            ("last workgroup skipped", False, r"fwd: unwritten: 896/"), ("last workgroup skipped", True, r"bwd: unwritten: 416/")]
    return [(f"unpatch-{d.replace(' ', '-')}-{'bwd' if b else 'fwd'}", functools.partial(_raises, functools.partial(_unpatch_host, geo, d, b), m))
            for d, b, m in rows]


# =========================================================================================== grouped pads
# (rows, s0, s1, d0, d1).  Destination totals, pad direction: 1, 255, 256, 257, 37632, 16, 315, 6912; unpad direction: 1, 15, 24, 200,
# 21168 (the 3x7x7x12 -> 16 mixer's gradient, 83 workgroups), 12, 315, 5184.
PAD_ENTRIES = [(1, 1, 1, 1, 1), (1, 3, 5, 15, 17), (4, 2, 3, 8, 8), (1, 1, 200, 1, 257), (147, 12, 12, 16, 16), (1, 1, 12, 1, 16), (5, 7, 9, 7, 9),
               (27, 12, 16, 16, 16)]
PAD_ORDERS = {"a": (0, 1, 2, 3, 4, 5, 6, 7), "b": (4, 7, 0, 6, 2, 5, 1, 3)}


def pad_starts(entries, unpad):
    starts, b = [], 0
    for r, s0, s1, d0, d1 in entries:
        starts.append(b)
        b += -(-(r * (s0 * s1 if unpad else d0 * d1)) // 256)
    return starts, b


@functools.lru_cache(maxsize=4)
def pad_case(order, unpad):
    k = _Case(order=order, unpad=unpad, entries=[PAD_ENTRIES[i] for i in PAD_ORDERS[order]], what=f"pads order {order} {'unpad' if unpad else 'pad'}")
    k.src, k.want = [], []
    for i, (r, s0, s1, d0, d1) in zip(PAD_ORDERS[order], k.entries):
        if unpad:
            src = patterns(r * d0 * d1, _seed("pad", i), torch.int32).view(r, d0, d1)
            want = src[:, :s0, :s1].contiguous()
        else:
            src = patterns(r * s0 * s1, _seed("pad", i), torch.int32).view(r, s0, s1)
            want = F.pad(src, (0, d1 - s1, 0, d0 - s0))
        k.src.append(src)
        k.want.append(want)
    k.starts, k.blocks = pad_starts(k.entries, unpad)
    # ---- validity
    assert len(k.entries) == 8
    totals = {u: sorted(r * (s0 * s1 if u else d0 * d1) for r, s0, s1, d0, d1 in PAD_ENTRIES) for u in (0, 1)}
    assert {1, 255, 256, 257, 6912} <= set(totals[0]) and {1, 21168} <= set(totals[1]) and -(-21168 // 256) == 83
    assert any(s0 == d0 and s1 == d1 and r * s0 * s1 > 1 for r, s0, s1, d0, d1 in PAD_ENTRIES)
    assert any((s0 == d0) != (s1 == d1) and s0 > 1 for r, s0, s1, d0, d1 in PAD_ENTRIES)
    other = pad_starts([PAD_ENTRIES[i] for i in PAD_ORDERS["b" if order == "a" else "a"]], unpad)[0]
    mine = dict(zip(PAD_ORDERS[order], k.starts))
    theirs = dict(zip(PAD_ORDERS["b" if order == "a" else "a"], other))
    assert all(mine[i] != theirs[i] for i in range(8)), f"{k.what}: an entry sits at the same block_start in both orders"
    return k


def cpu_pad(k, dst, defect=None):
    """pad_last2_grouped_kernel: one workgroup at a time, entry looked up by block_start."""
    n = len(k.entries)
    tid = torch.arange(256)
    for b in range(k.blocks):
        ei = 0
        for j in range(1, n):
            if (b > k.starts[j]) if defect == "entry boundary one workgroup off" else (b >= k.starts[j]):
                ei = j
        r, s0, s1, d0, d1 = k.entries[ei]
        src, out = k.src[ei].reshape(-1), dst.part(ei)
        i = (b - k.starts[ei]) * 256 + tid
        i = i[i < out.numel()]
        if not k.unpad:
            j_, q = i % d1, i // d1
            a, rr = q % d0, q // d0
            inside = (a < s0) & (j_ < s1)
            if defect != "zero fill missing":
                out[i[~inside]] = 0
            out[i[inside]] = src[((rr * s0 + a) * s1 + j_)[inside]]
        else:
            j_, q = i % s1, i // s1
            a, rr = q % s0, q // s0
            out[i] = src[(rr * d0 + a) * d1 + j_]


def _pad_host(order, unpad, defect=None):
    k = pad_case(order, unpad)
    dst = Packed([w.numel() for w in k.want], torch.int32, "cpu")
    cpu_pad(k, dst, defect)
    dst.check(k.want, k.what)


def _pad_defects():
    return [("pad-zero-fill-missing", functools.partial(_raises, functools.partial(_pad_host, "a", False, "zero fill missing"), r"pad: unwritten: ")),
            ("pad-entry-boundary-off-pad", functools.partial(_raises, functools.partial(_pad_host, "b", False, "entry boundary one workgroup off"), r"pad: unwritten: ")),
            ("pad-entry-boundary-off-unpad", functools.partial(_raises, functools.partial(_pad_host, "a", True, "entry boundary one workgroup off"), r"unpad: unwritten: "))]


# =========================================================================================== grouped transposes
TR_SEQ = [(64, 64), (768, 1536), (128, 320), (1536, 64), (64, 1536)]          # small and large entries alternate
TR_COUNTS = {1: 1, 2: 1, 64: 1, 65: 2, 130: 3}                                # pairs -> launches of ops.transpose_grouped


@functools.lru_cache(maxsize=1)
def tr_case(pairs):
    k = _Case(pairs=pairs, shapes=[TR_SEQ[i % len(TR_SEQ)] for i in range(pairs)], what=f"transposes {pairs}")
    k.src = [patterns(r * c, _seed("tr", i)).view(r, c) for i, (r, c) in enumerate(k.shapes)]
    k.want = [s.t().contiguous() for s in k.src]
    assert -(-pairs // 64) == TR_COUNTS[pairs] and all(r % 64 == 0 and c % 64 == 0 for r, c in k.shapes)
    assert pairs < 5 or {s for s in k.shapes} == set(TR_SEQ)
    return k


def cpu_transpose(k, dst, defect=None):
    """transpose_grouped_kernel tile by tile: dst tile (cj, ri) = src tile (ri, cj) transposed."""
    for i, ((r, c), src) in enumerate(zip(k.shapes, k.src)):
        tiles = src.view(r // 64, 64, c // 64, 64)
        inner = (2, 1, 0, 3) if defect == "tiles not transposed inside" else (2, 3, 0, 1)
        out = tiles.permute(*inner).reshape(c, r).clone()
        if defect == "first tile from the neighbour" and i % 64:
            out[:64, :64] = k.src[i - 1][:64, :64].t()
        dst.part(i).copy_(out.reshape(-1))


def _tr_host(pairs, defect=None):
    k = tr_case(pairs)
    dst = Packed([w.numel() for w in k.want], torch.int16, "cpu")
    cpu_transpose(k, dst, defect)
    dst.check(k.want, k.what)


def _tr_defects():
    return [("transpose-tiles-not-transposed-inside", functools.partial(_raises, functools.partial(_tr_host, 2, "tiles not transposed inside"), r"2: values: ")),
            ("transpose-first-tile-from-the-neighbour", functools.partial(_raises, functools.partial(_tr_host, 65, "first tile from the neighbour"), r"65: values: "))]


# =========================================================================================== SiLU stream
SILU_NVEC = 6 * (4096 * 256) + 1000
SILU_BLOCK = 4099 * 8


@functools.lru_cache(maxsize=1)
def silu_case():
    k = _Case(nvec=SILU_NVEC, n=SILU_NVEC * 8, what="silu stream")
    k.xb = (rnd((SILU_BLOCK,), 90) * 3).to(BF16)
    k.ref = F.silu(k.xb.double()).to(BF16)
    k.blocks = silu_blocks(k.nvec)
    assert k.blocks == SILU_CAP == 4096 and k.n == 50339648 and k.n % SILU_BLOCK
    s = k.blocks * 256
    assert [silu_trips(k.nvec, k.blocks, i) for i in (0, 999, 1000, s - 1)] == [(1, 3), (1, 3), (1, 2), (1, 2)]
    return k


def silu_input(k, device):
    reps = -(-k.n // SILU_BLOCK)
    return k.xb.to(device).repeat(reps)[:k.n].contiguous()


def cpu_silu(k, x, out, defect=None):
    y = F.silu(x.float()).to(BF16).view(torch.int16)
    n = min(k.n, 4 * k.blocks * 256 * 8) if defect == "tail loop skipped" else k.n      # every thread makes exactly one unrolled trip
    out.part(0)[:n] = y[:n]


def check_silu(k, out, what="silu stream"):
    body = out.part(0)
    p = POISON[torch.int16]
    rest = out.flat.clone()
    out.part(0, rest).fill_(p)
    bad = rest != p
    assert not bool(bad.any()), f"{what}: guards: {int(bad.sum())} elements behind n or in front of y changed"
    left = body == p
    assert not bool(left.any()), f"{what}: unwritten: {int(left.sum())}/{k.n} elements still hold the poison; first at {_first(left) if bool(left.any()) else -1}"
    full = k.n // SILU_BLOCK
    tiles = body[:full * SILU_BLOCK].view(full, SILU_BLOCK)
    differ = (tiles != tiles[0]).any(1)
    assert not bool(differ.any()), f"{what}: equal inputs, other bits: {int(differ.sum())}/{full} tiles differ from tile 0; first is tile {_first(differ) if bool(differ.any()) else -1}"
    tail = body[full * SILU_BLOCK:]
    assert torch.equal(tail, tiles[0][:tail.numel()]), f"{what}: equal inputs, other bits: the ragged last tile"
    assert_close(tiles[0].view(BF16), k.ref, rtol=2 ** -7, atol=1e-6, what=f"{what}: values")


def _silu_host(defect=None):
    k = silu_case()
    out = Packed([k.n], torch.int16, "cpu")
    cpu_silu(k, silu_input(k, "cpu"), out, defect)
    check_silu(k, out)


# =========================================================================================== what tests/test_host.py runs without a GPU
def _host_checks():
    out = [("mirrors", _mirrors_match_the_library), ("pool-second-sweep", _second_sweep_is_ragged)]
    out += [(i, functools.partial(_pool_host, make)) for i, make in _pool_makers()]
    out += [(f"unpatch-{'x'.join(map(str, g))}", functools.partial(_unpatch_host, g)) for g in UNPATCH]
    out += [(f"pads-{o}-{'unpad' if u else 'pad'}", functools.partial(_pad_host, o, u)) for o in PAD_ORDERS for u in (False, True)]
    out += [(f"transposes-{n}", functools.partial(_tr_host, n)) for n in TR_COUNTS]
    return out + [("silu", _silu_host)]


HOST_CHECKS = _host_checks()
DEFECT_CHECKS = (_pool_defects() + _unpatch_defects() + _pad_defects() + _tr_defects()
                 + [("silu-tail-loop-skipped", functools.partial(_raises, functools.partial(_silu_host, "tail loop skipped"), r"unwritten: 16785216/"))])


# =========================================================================================== the GPU side
def _err():
    from video_vae_amd._lib import VvaeError
    return VvaeError


def run_pool(k, dev):
    ops = _ops()
    bufs = pool_bufs(k, dev)
    for m in pool_modes(k):
        op, out = pool_out(k, m, dev)
        bufs[op] = out
        pool_regime(k, bufs, m, _lib())
        for o in POOL_OPS[m]:
            assert ops.rows(bufs[o].view)[0].data_ptr() == bufs[o].view.data_ptr(), f"{k.what}: {o} would be copied"
        if m == "fwd":
            ops.maxpool_fwd_raw(bufs["x"].view, out=out.view)
        else:
            ops.maxpool_bwd_raw(bufs["x"].view, bufs["dpool"].view, bufs["dskip"].view if m == "bwd1" else None, out=out.view)
        torch.cuda.synchronize()
        check_pool(k, out, m)
        del bufs[op], out


def test_mirrors_match_the_library():
    _mirrors_match_the_library()
    _second_sweep_is_ragged()


@pytest.mark.parametrize("family", ["I", "R"])
@pytest.mark.parametrize("geo,dtype,vw", SMALL_POOL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_max_pool_small(dev, geo, dtype, vw, family):
    run_pool(pool_case(family, geo, dtype, "contig", vw), dev)


@pytest.mark.parametrize("family", ["I", "R"])
@pytest.mark.parametrize("geo,dtype,layout,vw", PITCHED_POOL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_max_pool_pitched_slices(dev, geo, dtype, layout, vw, family):
    """Every operand a channel slice of a wider buffer, five different pitches (x the upper half of a 2C joint buffer); with and without
    dskip.  The complement of every input slice is NaN, of every output slice poison that must survive."""
    run_pool(pool_case(family, geo, dtype, layout, vw), dev)


@pytest.mark.parametrize("family", ["I", "R"])
@pytest.mark.parametrize("op,dtype", MIS_POOL, ids=str)
def test_max_pool_one_misaligned_operand(dev, op, dtype, family):
    """One operand at a time 8-byte aligned: vvae_pool_vec returns 1 for exactly that operand, the launch is scalar, the result exact."""
    run_pool(pool_case(family, (2, 3, 8, 6, 16), dtype, "mis-" + op, 8 if dtype == BF16 else 4), dev)


@pytest.mark.parametrize("family", ["I", "R"])
@pytest.mark.parametrize("geo,dtype,vw,blocks,trips", CAP_POOL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_max_pool_at_and_past_the_grid_cap(dev, geo, dtype, vw, blocks, trips, family):
    """The production launch (exactly 8192 workgroups, one trip each) and a ragged second trip of the scalar and of the vector form."""
    run_pool(pool_case(family, geo, dtype, "contig", vw, blocks, trips), dev)


@pytest.mark.parametrize("family", ["I", "R"])
@pytest.mark.parametrize("dtype,c", [(BF16, 16), (F32, 16), (BF16, 6), (F32, 6)], ids=str)
def test_max_pool_autograd_nodes(dev, dtype, c, family):
    """ops.max_pool_1x2x2 and ops.max_pool_fork with the cotangent of the pooled output only, of the skip only, and of both."""
    ops = _ops()
    k = pool_case(family, (2, 3, 8, 6, c), dtype, "contig", pool_vec(0, c, c, dtype))
    x, dpool, dskip = (v.to(dev, dtype) for v in (k.x, k.dpool, k.dskip))
    xa = x.clone().requires_grad_(True)
    y = ops.max_pool_1x2x2(xa)
    assert_exact(y.detach(), k.y, f"{k.what}: max_pool_1x2x2: y")
    (g,) = torch.autograd.grad(y, xa, dpool)
    assert_exact(g, k.dx0, f"{k.what}: max_pool_1x2x2: dx")
    for name, want in (("pool", k.dx0), ("skip", k.dskip.to(dtype)), ("both", k.dx1)):
        xa = x.clone().requires_grad_(True)
        pooled, skip = ops.max_pool_fork(xa)
        assert_exact(pooled.detach(), k.y, f"{k.what}: max_pool_fork: y")
        assert torch.equal(skip.detach().view(INT[dtype]), x.view(INT[dtype])), "the skip is x itself"
        outs, gs = {"pool": ([pooled], [dpool]), "skip": ([skip], [dskip]), "both": ([pooled, skip], [dpool, dskip])}[name]
        (g,) = torch.autograd.grad(outs, xa, gs)
        assert_exact(g, want, f"{k.what}: max_pool_fork, cotangent of {name}: dx")


def _pool_lib_call(k, bufs, mode, dims=None, ld=None):
    n, t, h, w, c = dims or k.geo
    ld = {op: (ld or {}).get(op, bufs[op].width) for op in bufs}
    p = {op: ctypes.c_void_p(bufs[op].view.data_ptr()) for op in bufs}
    ops = _ops()
    if mode == "fwd":
        return _lib().vvae_maxpool_1x2x2_fwd(p["x"], ld["x"], p["y"], ld["y"], n * t, h, w, c, DT[k.dtype], ops._stream())
    return _lib().vvae_maxpool_1x2x2_bwd(p["x"], ld["x"], p["dpool"], ld["dpool"], p["dskip"], ld["dskip"], p["dx"], ld["dx"], n * t, h, w, c,
                                         DT[k.dtype], ops._stream())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=str)
def test_max_pool_refusals(dev, dtype):
    """Odd H, odd W and a pitch below C for each operand raise VvaeError and write nothing."""
    from video_vae_amd._lib import check
    k = pool_case("I", (2, 3, 8, 6, 16), dtype, "contig", 8 if dtype == BF16 else 4)
    bufs = pool_bufs(k, dev)
    bufs["y"], bufs["dx"] = pool_out(k, "fwd", dev)[1], pool_out(k, "bwd1", dev)[1]
    assert _pool_lib_call(k, bufs, "fwd") == 0 and _pool_lib_call(k, bufs, "bwd1") == 0        # the calls themselves are well formed
    bufs["y"], bufs["dx"] = pool_out(k, "fwd", dev)[1], pool_out(k, "bwd1", dev)[1]
    bad = [("fwd", dict(dims=(2, 3, 7, 6, 16))), ("fwd", dict(dims=(2, 3, 8, 5, 16))), ("bwd1", dict(dims=(2, 3, 7, 6, 16))),
           ("bwd1", dict(dims=(2, 3, 8, 5, 16)))]
    bad += [("fwd", dict(ld={op: 15})) for op in ("x", "y")] + [("bwd1", dict(ld={op: 15})) for op in ("x", "dpool", "dskip", "dx")]
    for mode, kw in bad:
        with pytest.raises(_err()):
            check(_pool_lib_call(k, bufs, mode, **kw), f"{mode} {kw}")
    ops = _ops()
    for shape in ((2, 3, 7, 6, 16), (2, 3, 8, 5, 16)):                                         # and through the raw entries of ops
        xo = torch.zeros(shape, dtype=dtype, device=dev)
        with pytest.raises(_err()):
            ops.maxpool_fwd_raw(xo, out=bufs["y"].view)
        with pytest.raises(_err()):
            ops.maxpool_bwd_raw(xo, bufs["dpool"].view, bufs["dskip"].view, out=bufs["dx"].view)
    torch.cuda.synchronize()
    bufs["y"].untouched("pool refusals: y")
    bufs["dx"].untouched("pool refusals: dx")


@pytest.mark.parametrize("geo", UNPATCH, ids=lambda g: "x".join(map(str, g)))
def test_unpatch_pad_bitwise(dev, geo):
    """ops.unpatch_pad both ways on bit patterns: the forward zero-fills the pad channels, the backward ignores the NaN patterns in the pad
    channels of g and writes every element of a poisoned gx; the guards around both stay."""
    ops = _ops()
    k = unpatch_case(geo)
    f, h, w, p, cu, c = geo
    for backward in (False, True):
        src, dst = _unpatch_bufs(k, backward, dev)
        ops.unpatch_pad(src.part(0).view(BF16), dst.part(0).view(BF16), f, h, w, p, cu, c, backward)
        torch.cuda.synchronize()
        dst.check([k.gx if backward else k.y], f"{k.what}: {'bwd' if backward else 'fwd'}")
        src.check([k.g if backward else k.x], f"{k.what}: the source of {'bwd' if backward else 'fwd'}")


def test_unpatch_pad_refusals(dev):
    """cu or c not a multiple of 4, c < cu, a pointer off by one element, fp32: VvaeError, and the destination stays as it was."""
    ops = _ops()
    src = Packed([4096], torch.int16, dev, [patterns(4096, 5).to(dev)])
    dst = Packed([4096], torch.int16, dev)
    s, d = src.part(0).view(BF16), dst.part(0).view(BF16)
    ops.unpatch_pad(s, Packed([4096], torch.int16, dev).part(0).view(BF16), 1, 2, 3, 2, 4, 8, False)     # well formed: 1*2*3*4*4 = 96 in, 192 out
    off_s, off_d = src.flat[src.offs[0] + 1:].view(BF16), dst.flat[dst.offs[0] + 1:].view(BF16)
    for backward in (False, True):
        for args in ((s, d, 1, 2, 3, 2, 6, 8), (s, d, 1, 2, 3, 2, 4, 6), (s, d, 1, 2, 3, 2, 8, 4), (off_s, d, 1, 2, 3, 2, 4, 8), (s, off_d, 1, 2, 3, 2, 4, 8)):
            with pytest.raises(_err()):
                ops.unpatch_pad(*args, backward)
        with pytest.raises(_err()):
            ops.unpatch_pad(torch.zeros(4096, device=dev), dst.flat[dst.offs[0]:].view(BF16).view(F32), 1, 2, 3, 2, 4, 8, backward)
    torch.cuda.synchronize()
    dst.untouched("unpatch refusals")


def _pad_call(srcs, dsts, entries, unpad):
    n = len(srcs)
    VP, LA, IA = ctypes.c_void_p * n, ctypes.c_long * n, ctypes.c_int * n
    col = lambda j: IA(*[e[j] for e in entries])
    return _lib().vvae_pad_last2_grouped(VP(*[t.data_ptr() for t in srcs]), VP(*[t.data_ptr() for t in dsts]), LA(*[e[0] for e in entries]),
                                         col(1), col(2), col(3), col(4), n, 1 if unpad else 0, _ops()._stream())


@pytest.mark.parametrize("unpad", [False, True], ids=["pad", "unpad"])
@pytest.mark.parametrize("order", list(PAD_ORDERS))
def test_pad_last2_grouped_bitwise(dev, order, unpad):
    """vvae_pad_last2_grouped with the maximum of 8 entries, in two orders (every entry at another block_start), both directions, into
    NaN-filled destinations packed with guards between them."""
    k = pad_case(order, unpad)
    srcs = [s.to(dev).view(F32) for s in k.src]
    dst = Packed([w.numel() for w in k.want], torch.int32, dev)
    assert _pad_call(srcs, [dst.part(i).view(F32) for i in range(8)], k.entries, unpad) == 0
    torch.cuda.synchronize()
    dst.check(k.want, k.what)


def test_pad_last2_grouped_refusals(dev):
    """Nine tensors, and an entry with s > d in either dim: status 1001 (VvaeError through check), nothing written."""
    from video_vae_amd._lib import check
    k = pad_case("a", False)
    srcs = [s.to(dev).view(F32) for s in k.src]
    dst = Packed([w.numel() for w in k.want] + [1], torch.int32, dev)
    parts = [dst.part(i).view(F32) for i in range(9)]
    calls = [(srcs + [srcs[0]], parts, k.entries + [k.entries[0]], False)]
    for j, e in ((1, (1, 16, 5, 15, 17)), (1, (1, 3, 18, 15, 17))):
        calls.append((srcs, parts[:8], k.entries[:j] + [e] + k.entries[j + 1:], False))
        calls.append((srcs, parts[:8], k.entries[:j] + [e] + k.entries[j + 1:], True))
    for a in calls:
        rc = _pad_call(*a)
        assert rc == 1001, rc
        with pytest.raises(_err()):
            check(rc, "vvae_pad_last2_grouped")
    with pytest.raises(_err()):
        _ops().pad_last2_group([s.clone() for s in srcs] + [srcs[0].clone()], [(e[3], e[4]) for e in k.entries] + [(1, 1)])
    torch.cuda.synchronize()
    dst.untouched("pad refusals")


def test_pad_last2_group_autograd_with_an_absent_cotangent(dev):
    """ops.pad_last2_group == F.pad bitwise for 8 parameters (a 5-D kernel, a vector, an unpadded one ...); in the backward one output has
    no cotangent: its parameter gets None, the others the corner of their cotangent, bitwise."""
    ops = _ops()
    shapes = [((3, 7, 7, 12, 12), (16, 16)), ((12,), (16,)), ((3, 3, 3, 12, 16), (16, 16)), ((1, 1), (1, 1)), ((5, 7, 9), (7, 9)), ((3, 5), (15, 17)),
              ((4, 2, 3), (8, 8)), ((200,), (257,))]
    params = [rnd(s, 300 + i).to(dev).requires_grad_(True) for i, (s, _) in enumerate(shapes)]
    outs = ops.pad_last2_group(params, [t for _, t in shapes])
    gs = []
    for i, (p, o, (s, t)) in enumerate(zip(params, outs, shapes)):
        pad = (0, t[-1] - s[-1]) if len(t) == 1 else (0, t[1] - s[-1], 0, t[0] - s[-2])
        assert torch.equal(o.detach().view(torch.int32), F.pad(p.detach(), pad).view(torch.int32)), f"pad_last2_group: output {i}"
        gs.append(rnd(tuple(o.shape), 400 + i).to(dev))
    keep = [i for i in range(8) if i != 2]
    grads = torch.autograd.grad([outs[i] for i in keep], params, [gs[i] for i in keep], allow_unused=True)
    for i, (gr, (s, t)) in enumerate(zip(grads, shapes)):
        if i == 2:
            assert gr is None, "an output without a cotangent must give its parameter None"
            continue
        want = gs[i][..., :s[-1]] if len(t) == 1 else gs[i][..., :s[-2], :s[-1]]
        assert gr.shape == params[i].shape and torch.equal(gr.view(torch.int32), want.contiguous().view(torch.int32)), f"pad_last2_group: gradient {i}"


@pytest.mark.parametrize("pairs", list(TR_COUNTS))
def test_transpose_grouped_bitwise(dev, pairs):
    """ops.transpose_grouped over 1, 2, 64, 65 and 130 pairs (one, two and three launches; the 64-entry start[] search full at 64), small and
    large matrices alternating: every dst equals src.t() bitwise, the guards between the poisoned destinations stay."""
    ops = _ops()
    k = tr_case(pairs)
    src = Packed([s.numel() for s in k.src], torch.int16, "cpu", k.src).to(dev)
    dst = Packed([w.numel() for w in k.want], torch.int16, dev)
    ops.transpose_grouped([(src.part(i).view(BF16).view(r, c), dst.part(i).view(BF16).view(c, r)) for i, (r, c) in enumerate(k.shapes)])
    torch.cuda.synchronize()
    dst.check(k.want, k.what)
    src.check([s.contiguous() for s in k.src], f"{k.what}: the sources")


def test_transpose_grouped_refusals(dev):
    """A dimension that is no multiple of 64 and a pointer that is not 16-byte aligned: VvaeError, nothing written (the good entry in front
    of the bad one neither)."""
    ops = _ops()
    src = Packed([64 * 64, 64 * 96 + 8], torch.int16, dev)
    dst = Packed([64 * 64, 64 * 96 + 8], torch.int16, dev)
    src.flat.copy_(patterns(src.flat.numel(), 9).to(dev))
    good = (src.part(0).view(BF16).view(64, 64), dst.part(0).view(BF16).view(64, 64))
    for bad in ((src.part(1)[:64 * 96].view(BF16).view(64, 96), dst.part(1)[:64 * 96].view(BF16).view(96, 64)),
                (src.part(1)[:64 * 96].view(BF16).view(96, 64), dst.part(1)[:64 * 96].view(BF16).view(64, 96)),
                (src.part(1)[4:4 + 4096].view(BF16).view(64, 64), dst.part(1)[:4096].view(BF16).view(64, 64)),
                (src.part(1)[:4096].view(BF16).view(64, 64), dst.part(1)[4:4 + 4096].view(BF16).view(64, 64))):
        with pytest.raises(_err()):
            ops.transpose_grouped([good, bad])
    torch.cuda.synchronize()
    dst.untouched("transpose refusals")


def test_silu_stream_past_the_grid_cap(dev):
    """vvae_silu_bf16 over 6 * (4096 * 256) + 1000 vectors: 4096 workgroups (the cap), one unrolled trip and two or three tail trips per
    thread, the last one ragged; the values at test_silu_stream_kernel's bar, equal inputs giving equal bits, the output poisoned first,
    the guards behind n unchanged."""
    from video_vae_amd._lib import check
    k = silu_case()
    assert _lib().vvae_silu_blocks(k.nvec) == k.blocks == 4096
    x = silu_input(k, dev)
    out = Packed([k.n], torch.int16, dev)
    assert x.data_ptr() % 16 == 0 and out.part(0).data_ptr() % 16 == 0
    check(_lib().vvae_silu_bf16(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.part(0).data_ptr()), k.n, _ops()._stream()), "vvae_silu_bf16")
    torch.cuda.synchronize()
    check_silu(k, out)
