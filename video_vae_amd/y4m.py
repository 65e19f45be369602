"""YUV4MPEG2 (``.y4m``) clips: the container and the colour arithmetic, in numpy only.  This module is the specification of
csrc/yuv.hip (ops.yuv_to_rgb_u8 / ops.rgb_to_yuv), which computes the same bytes on the device.

Container.  The stream header is one line, ``YUV4MPEG2 W<w> H<h> [F<n>:<d>] [I<c>] [A<n>:<d>] [C<tag>] [X<anything>]...\\n``: tokens
separated by single spaces, in any order after the magic.  Every frame is a line ``FRAME[ params]\\n`` (at most 80 bytes) followed by the
planes Y (H x W bytes), then U and V (CH x CW each: CH = (H + 1) // 2, CW = (W + 1) // 2 for 4:2:0, H x W for 4:4:4, none for mono).
The frames are found by walking the FRAME lines; their lengths may differ.

  accepted: C420, C420jpeg, no C tag (4:2:0, chroma sited at the centre of its 2 x 2 luma block); C420mpeg2 (4:2:0, horizontally
            co-sited with the even luma columns); C444; Cmono; Ip, I?, no I tag; XCOLORRANGE=FULL / XCOLORRANGE=LIMITED (any other X
            tag and A are ignored).
  refused (ValueError naming the file and the tag): C420paldv, C422, C411, C444alpha, every tag with a bit depth (...p10, p12, p16) and
            any other C tag; It, Ib, Im; a missing W or H, a side above 16384; a FRAME line that is not there; a last frame cut short.

Colour arithmetic.  int32 throughout, ``>>`` an arithmetic shift (floor).  A matrix is bt601 or bt709, a range limited (off = 16) or full
(off = 0); COEFFS holds, times 2^14, the forward rows (ry gy by / ru gu bu / rv gv bv) and the inverse (cy crv cgu cgv cbu).  gy, gu and
gv are remainders, so greys map to U = V = 128 exactly and white to 235 (limited) or 255 (full).

  to RGB.  The chroma of luma pixel (y, x) is taken at 4 extra bits.  4:2:0: U16 = sum wv[i] wh[j] U[r_i][c_j] (likewise V16).  Rows are
  always centre-sited: r0 = y >> 1, r1 = r0 + 1 when y is odd, else r0 - 1, clamped to 0 .. CH - 1, wv = (3, 1).  Columns, centre
  siting: the same rule with x and CW, wh = (3, 1).  Columns, C420mpeg2: c0 = x >> 1, c1 = min(c0 + 1, CW - 1), wh = (4, 0) for even x and
  (2, 2) for odd x.  4:4:4: U16 = 16 U.  mono: U16 = V16 = 2048.  Then with u = U16 - 2048, v = V16 - 2048, l = 16 cy (Y - off):
      R = clip((l + crv v + 2^17) >> 18), G = clip((l + cgu u + cgv v + 2^17) >> 18), B = clip((l + cbu u + 2^17) >> 18), clip to 0 .. 255.
  No intermediate exceeds 1.5e8 in magnitude.

  from RGB (the writer's forms: 4:2:0 centre siting, tagged C420jpeg, and C444).  Y = clip((ry R + gy G + by B + (off << 14) + 2^13) >> 14).
  4:2:0: with a the sum of ru R + gu G + bu B over the pixel's 2 x 2 block, U = clip((a + (128 << 16) + 2^15) >> 16) (likewise V); a block
  index past the right or bottom edge of an odd frame reads the edge pixel again, so a block always has four terms.  4:4:4: the same
  expression with the one pixel counted four times.

Over all 2^24 colours a constant-colour frame taken RGB -> YUV -> RGB comes back within 2 per channel in the limited ranges and within 1
in the full ranges; greys come back with R = G = B, within 1 (limited) and exactly (full).

Windows (the training loader's device path; csrc/yuv_window.hip computes window_to_rgb_reference's bytes).  A window is the luma crop
[top, top + h) x [left, left + w) of some frames together with the chroma it needs: y (n, h, w); 4:2:0: u, v (n, h // 2 + 3, w // 2 + 3),
window row k = chroma row clamp((top >> 1) - 1 + k, 0, CH - 1) of the file, columns likewise with left and CW; 4:4:4: the same crop as y;
mono: none.  The clamped gather is the edge replication of the to-RGB rule above, so inside a window nothing is clamped and only the
parities (top & 1, left & 1) are needed: luma row y' of the crop is frame-parity row Y = (top & 1) + y', its taps r0 = (Y >> 1) + 1 and
r0 + 1 (Y odd) or r0 - 1 (Y even); columns the same (mpeg2: c0 = (X >> 1) + 1, c1 = c0 + 1).  The largest index used is
((1 + h - 1) >> 1) + 2 <= h // 2 + 2, which is why the window has h // 2 + 3 rows for every parity of top and h.
Padding value: a frame that must come out as RGB (0, 0, 0) is Y = 16 (limited) or Y = 0 (full) with U = V = 128: l = 0, u = v = 0 and so
R = G = B = (2^17) >> 18 = 0 exactly, in every matrix and range.
"""
import os
from dataclasses import dataclass, field

import numpy as np

MAGIC = b"YUV4MPEG2"
MAX_SIDE = 16384
MAX_LINE = 80                    # a FRAME line, its newline included
MAX_HEADER = 4096                # the stream header line
MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")
CHROMAS = ("420", "444", "mono")
SITINGS = ("centre", "mpeg2")

# (matrix, full) -> (forward 3 x 3 rows ry gy by / ru gu bu / rv gv bv, inverse cy crv cgu cgv cbu), all times 2^14
COEFFS = {
    ("bt601", False): (((4207, 8260, 1604), (-2428, -4768, 7196), (7196, -6026, -1170)), (19077, 26149, -6419, -13320, 33050)),
    ("bt601", True): (((4899, 9617, 1868), (-2765, -5427, 8192), (8192, -6860, -1332)), (16384, 22970, -5638, -11700, 29032)),
    ("bt709", False): (((2991, 10064, 1016), (-1649, -5547, 7196), (7196, -6536, -660)), (19077, 29372, -3494, -8731, 34610)),
    ("bt709", True): (((3483, 11718, 1183), (-1877, -6315, 8192), (8192, -7441, -751)), (16384, 25802, -3069, -7670, 30402)),
}

# C tag -> (chroma, siting)
_C_TAGS = {"420": ("420", "centre"), "420jpeg": ("420", "centre"), "420mpeg2": ("420", "mpeg2"), "444": ("444", "centre"),
           "mono": ("mono", "centre")}
_WRITE_TAGS = {"420": "420jpeg", "444": "444", "mono": "mono"}


def _coeffs(matrix, full):
    if matrix not in MATRICES:
        raise ValueError(f"matrix {matrix!r}: one of {MATRICES}")
    return COEFFS[(matrix, bool(full))]


def chroma_shape(h, w, chroma):
    """(CH, CW) of a chroma plane of an h x w frame; (0, 0) for mono."""
    if chroma == "420":
        return (h + 1) // 2, (w + 1) // 2
    if chroma == "444":
        return h, w
    if chroma == "mono":
        return 0, 0
    raise ValueError(f"chroma {chroma!r}: one of {CHROMAS}")


@dataclass
class Y4MHeader:
    """The stream header of a .y4m file.  ``full`` is None when the file carries no XCOLORRANGE tag; ``size`` is the header line's length
    in bytes, its newline included: the first FRAME line starts there."""
    width: int
    height: int
    fps: tuple = (0, 0)
    interlace: str = "?"
    aspect: tuple = (0, 0)
    chroma: str = "420"
    siting: str = "centre"
    full: object = None
    tag: str = ""
    extra: list = field(default_factory=list)
    size: int = 0

    @property
    def chroma_shape(self):
        return chroma_shape(self.height, self.width, self.chroma)

    @property
    def frame_bytes(self):
        ch, cw = self.chroma_shape
        return self.height * self.width + 2 * ch * cw


def _ratio(path, token):
    try:
        n, d = token[1:].split(":")
        return int(n), int(d)
    except ValueError:
        raise ValueError(f"{path}: tag {token!r} is not {token[:1]}<n>:<d>")


def parse_header(line, path="<y4m>"):
    """The header line (bytes, without or with its newline) -> Y4MHeader (``size`` = the line's length plus the newline)."""
    body = line[:-1] if line.endswith(b"\n") else line
    try:
        tokens = body.decode("ascii").split(" ")
    except UnicodeDecodeError:
        raise ValueError(f"{path}: the stream header is not ASCII")
    if tokens[0] != MAGIC.decode():
        raise ValueError(f"{path}: not a YUV4MPEG2 stream (the file starts with {body[:9]!r})")
    h = Y4MHeader(width=0, height=0, size=len(body) + 1)
    for tok in tokens[1:]:
        if not tok:
            continue
        key, val = tok[0], tok[1:]
        if key in "WH":
            if not val.isdigit():
                raise ValueError(f"{path}: tag {tok!r} is not a size")
            if key == "W":
                h.width = int(val)
            else:
                h.height = int(val)
        elif key == "F":
            h.fps = _ratio(path, tok)
        elif key == "A":
            h.aspect = _ratio(path, tok)
        elif key == "I":
            if val not in ("p", "?"):
                raise ValueError(f"{path}: tag {tok!r}: interlaced streams are not supported (Ip, I? or no I tag)")
            h.interlace = val
        elif key == "C":
            if val not in _C_TAGS:
                raise ValueError(f"{path}: tag {tok!r}: chroma format not supported (C420, C420jpeg, C420mpeg2, C444, Cmono, 8 bits)")
            h.tag = val
            h.chroma, h.siting = _C_TAGS[val]
        elif key == "X":
            if val == "COLORRANGE=FULL":
                h.full = True
            elif val == "COLORRANGE=LIMITED":
                h.full = False
            h.extra.append(tok)
        else:
            raise ValueError(f"{path}: tag {tok!r} is not a YUV4MPEG2 header tag")
    for key, side in (("W", h.width), ("H", h.height)):
        if side < 1:
            raise ValueError(f"{path}: the stream header has no {key} tag")
        if side > MAX_SIDE:
            raise ValueError(f"{path}: tag {key}{side}: a side above {MAX_SIDE}")
    return h


def read_header(path):
    """The Y4MHeader of the file at ``path``."""
    with open(path, "rb") as fh:
        head = fh.read(MAX_HEADER)
    end = head.find(b"\n")
    if end < 0:
        raise ValueError(f"{path}: no stream header line in the first {MAX_HEADER} bytes")
    return parse_header(head[:end + 1], path)


def _weights_420(n, cn, siting):
    """One axis of the 4:2:0 upsampling, luma extent ``n``, chroma extent ``cn``: (i0, i1 taps, w0, w1 weights summing to 4), each (n,)."""
    i = np.arange(n, dtype=np.int32)
    i0 = i >> 1
    odd = (i & 1) == 1
    if siting == "centre":
        i1 = np.clip(np.where(odd, i0 + 1, i0 - 1), 0, cn - 1).astype(np.int32)
        return i0, i1, np.full(n, 3, np.int32), np.full(n, 1, np.int32)
    if siting == "mpeg2":
        i1 = np.minimum(i0 + 1, cn - 1).astype(np.int32)
        return i0, i1, np.where(odd, 2, 4).astype(np.int32), np.where(odd, 2, 0).astype(np.int32)
    raise ValueError(f"siting {siting!r}: one of {SITINGS}")


def _chroma16(c, h, w, chroma, siting):
    """A chroma plane (T, CH, CW) uint8 -> its value at every luma pixel with 4 extra bits, int32 (T, h, w)."""
    c = np.asarray(c).astype(np.int32)
    if chroma == "444":
        return 16 * c
    r0, r1, a0, a1 = _weights_420(h, c.shape[1], "centre")
    c0, c1, b0, b1 = _weights_420(w, c.shape[2], siting)
    tap = lambda r, q: c[:, r[:, None], q[None, :]]
    a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[None, None, :], b1[None, None, :]
    return a0 * (b0 * tap(r0, c0) + b1 * tap(r0, c1)) + a1 * (b0 * tap(r1, c0) + b1 * tap(r1, c1))


def _check_planes(y, u, v, chroma):
    y = np.asarray(y)
    if y.ndim != 3 or y.dtype != np.uint8:
        raise ValueError(f"expected uint8 luma (T, H, W), got {y.dtype} {y.shape}")
    t, h, w = y.shape
    if chroma == "mono":
        return y, None, None
    want = (t,) + chroma_shape(h, w, chroma)
    u, v = np.asarray(u), np.asarray(v)
    for name, p in (("U", u), ("V", v)):
        if p.dtype != np.uint8 or p.shape != want:
            raise ValueError(f"expected uint8 {name} plane {want} for {chroma} frames of {h}x{w}, got {p.dtype} {p.shape}")
    return y, u, v


def yuv_to_rgb_reference(y, u, v, chroma="420", siting="centre", matrix="bt601", full=False):
    """Planes uint8 y (T, H, W), u and v (T, CH, CW) (ignored for mono) -> uint8 RGB (T, H, W, 3): the module's to-RGB arithmetic."""
    y, u, v = _check_planes(y, u, v, chroma)
    if siting not in SITINGS:
        raise ValueError(f"siting {siting!r}: one of {SITINGS}")
    _, (cy, crv, cgu, cgv, cbu) = _coeffs(matrix, full)
    t, h, w = y.shape
    off = 0 if full else 16
    l = 16 * cy * (y.astype(np.int32) - off)
    if chroma == "mono":
        uu = vv = np.zeros((t, h, w), dtype=np.int32)
    else:
        uu = _chroma16(u, h, w, chroma, siting) - 2048
        vv = _chroma16(v, h, w, chroma, siting) - 2048
    half = np.int32(1 << 17)
    r = (l + crv * vv + half) >> 18
    g = (l + cgu * uu + cgv * vv + half) >> 18
    b = (l + cbu * uu + half) >> 18
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def rgb_to_yuv_reference(rgb, chroma="420", matrix="bt601", full=False):
    """uint8 RGB (T, H, W, 3) -> planes uint8 (y (T, H, W), u, v (T, CH, CW)): the module's from-RGB arithmetic, 4:2:0 centre siting or
    4:4:4."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 4 or rgb.shape[-1] != 3 or rgb.dtype != np.uint8:
        raise ValueError(f"expected uint8 RGB (T, H, W, 3), got {rgb.dtype} {rgb.shape}")
    if chroma not in ("420", "444"):
        raise ValueError(f"chroma {chroma!r}: the writer's forms are '420' and '444'")
    (ry, gy, by), (ru, gu, bu), (rv, gv, bv) = _coeffs(matrix, full)[0]
    t, h, w, _ = rgb.shape
    off = 0 if full else 16
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    y = (ry * r + gy * g + by * b + (off << 14) + (1 << 13)) >> 14
    cu = ru * r + gu * g + bu * b
    cv = rv * r + gv * g + bv * b
    if chroma == "444":
        au, av = 4 * cu, 4 * cv
    else:
        ch, cw = chroma_shape(h, w, chroma)
        rows = np.minimum(np.arange(2 * ch), h - 1)
        cols = np.minimum(np.arange(2 * cw), w - 1)
        block = lambda c: c[:, rows[:, None], cols[None, :]].reshape(t, ch, 2, cw, 2).sum(axis=(2, 4), dtype=np.int32)
        au, av = block(cu), block(cv)
    bias = (128 << 16) + (1 << 15)
    clip = lambda x: np.clip(x, 0, 255).astype(np.uint8)
    return clip(y), clip((au + bias) >> 16), clip((av + bias) >> 16)


PAD_CHROMA = 128


def pad_luma(full):
    """The luma byte of the padding value (module docstring): with U = V = PAD_CHROMA it converts to RGB (0, 0, 0) exactly."""
    return 0 if full else 16


def window_chroma_shape(h, w, chroma):
    """(rows, columns) of the chroma planes of a window whose luma crop is h x w; (0, 0) for mono."""
    if chroma == "420":
        return h // 2 + 3, w // 2 + 3
    if chroma == "444":
        return h, w
    if chroma == "mono":
        return 0, 0
    raise ValueError(f"chroma {chroma!r}: one of {CHROMAS}")


def _window_weights(n, parity, siting):
    """_weights_420 inside a window: luma index i of the crop is frame-parity index parity + i; nothing is clamped."""
    i = np.arange(n, dtype=np.int32) + np.int32(parity)
    i0 = (i >> 1) + 1
    odd = (i & 1) == 1
    if siting == "centre":
        return i0, np.where(odd, i0 + 1, i0 - 1).astype(np.int32), np.full(n, 3, np.int32), np.full(n, 1, np.int32)
    if siting == "mpeg2":
        return i0, i0 + 1, np.where(odd, 2, 4).astype(np.int32), np.where(odd, 2, 0).astype(np.int32)
    raise ValueError(f"siting {siting!r}: one of {SITINGS}")


def window_to_rgb_reference(y, u, v, parity=(0, 0), chroma="420", siting="centre", matrix="bt601", full=False):
    """A window (Y4MClip.window: y (n, h, w), u and v of window_chroma_shape, None for mono) with ``parity`` = (top & 1, left & 1) -> uint8
    RGB (n, h, w, 3): the module's to-RGB arithmetic on a window.  It equals yuv_to_rgb_reference(whole planes)[:, top:top + h,
    left:left + w] and is the specification of csrc/yuv_window.hip's conversion."""
    y = np.asarray(y)
    if y.ndim != 3 or y.dtype != np.uint8:
        raise ValueError(f"expected uint8 luma (n, h, w), got {y.dtype} {y.shape}")
    if siting not in SITINGS:
        raise ValueError(f"siting {siting!r}: one of {SITINGS}")
    n, h, w = y.shape
    _, (cy, crv, cgu, cgv, cbu) = _coeffs(matrix, full)
    l = 16 * cy * (y.astype(np.int32) - (0 if full else 16))
    if chroma == "mono":
        uu = vv = np.zeros((n, h, w), dtype=np.int32)
    else:
        want = (n,) + window_chroma_shape(h, w, chroma)
        planes = []
        for name, c in (("U", u), ("V", v)):
            c = np.asarray(c)
            if c.dtype != np.uint8 or c.shape != want:
                raise ValueError(f"expected uint8 {name} window {want} for a {chroma} crop of {h}x{w}, got {c.dtype} {c.shape}")
            c = c.astype(np.int32)
            if chroma == "444":
                planes.append(16 * c - 2048)
                continue
            r0, r1, a0, a1 = _window_weights(h, int(parity[0]) & 1, "centre")
            c0, c1, b0, b1 = _window_weights(w, int(parity[1]) & 1, siting)
            tap = lambda r, q: c[:, r[:, None], q[None, :]]
            a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[None, None, :], b1[None, None, :]
            planes.append(a0 * (b0 * tap(r0, c0) + b1 * tap(r0, c1)) + a1 * (b0 * tap(r1, c0) + b1 * tap(r1, c1)) - 2048)
        uu, vv = planes
    half = np.int32(1 << 17)
    r = (l + crv * vv + half) >> 18
    g = (l + cgu * uu + cgv * vv + half) >> 18
    b = (l + cbu * uu + half) >> 18
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


class Y4MClip:
    """A .y4m file as a clip of uint8 RGB frames: ``shape`` = (T, H, W, 3); ``clip[a:b]`` converts frames [a, b) on the host
    (yuv_to_rgb_reference); ``planes(a, b)`` / ``records(a, b)`` hand out views of the memory-mapped file, nothing copied.
    ``matrix``: the container carries none.  ``range``: "header" (limited unless the file says XCOLORRANGE=FULL), "limited" or "full"."""

    def __init__(self, path, matrix="bt601", range="header"):
        if matrix not in MATRICES:
            raise ValueError(f"{path}: matrix {matrix!r}: one of {MATRICES}")
        if range not in ("header",) + RANGES:
            raise ValueError(f"{path}: range {range!r}: one of ('header',) + {RANGES}")
        self.path, self.matrix = path, matrix
        self.header = h = read_header(path)
        self.full = bool(h.full) if range == "header" else range == "full"
        self.chroma, self.siting = h.chroma, h.siting
        size = os.path.getsize(path)
        self.mm = np.memmap(path, dtype=np.uint8, mode="r") if size else np.zeros((0,), dtype=np.uint8)
        starts, lines = [], []
        pos, fb = h.size, h.frame_bytes
        while pos < size:
            line = bytes(self.mm[pos:pos + MAX_LINE])
            end = line.find(b"\n")
            if not line.startswith(b"FRAME") or end < 0 or (end > 5 and line[5:6] != b" "):
                raise ValueError(f"{path}: no FRAME line at byte {pos} (frame {len(starts)})")
            if pos + end + 1 + fb > size:
                raise ValueError(f"{path}: frame {len(starts)} is cut short: {size - pos - end - 1} of {fb} bytes")
            starts.append(pos)
            lines.append(end + 1)
            pos += end + 1 + fb
        self.starts = np.asarray(starts, dtype=np.int64)          # of the FRAME lines
        self.lines = np.asarray(lines, dtype=np.int64)            # their lengths
        self.shape = (len(starts), h.height, h.width, 3)
        self.ndim, self.dtype = 4, np.dtype(np.uint8)

    def __len__(self):
        return self.shape[0]

    def runs(self, a=0, b=None, run_bytes=None):
        """[(s, e)] covering frames [a, b): inside a run every FRAME line has the same length, so its records lie at one stride; with
        ``run_bytes`` a run holds at most about that many bytes (at least one frame)."""
        b = self.shape[0] if b is None else min(b, self.shape[0])
        per = None if run_bytes is None else max(1, int(run_bytes) // (self.header.frame_bytes + MAX_LINE))
        out, s = [], max(a, 0)
        while s < b:
            e = s + 1
            while e < b and self.lines[e] == self.lines[s] and (per is None or e - s < per):
                e += 1
            out.append((s, e))
            s = e
        return out

    def records(self, a, b):
        """(bytes of the frame records [a, b) as they lie in the file, a 1-D view; the length of their FRAME lines; the record stride).
        [a, b) must be one of ``runs``: equal FRAME lines."""
        if not 0 <= a < b <= self.shape[0] or (self.lines[a:b] != self.lines[a]).any():
            raise ValueError(f"{self.path}: frames [{a}, {b}) are not one run of equal FRAME lines (see runs())")
        line = int(self.lines[a])
        stride = line + self.header.frame_bytes
        s = int(self.starts[a])
        return self.mm[s:s + (b - a) * stride], line, stride

    def plane_views(self, buf, n, line, stride):
        """The planes (y, u, v) of ``n`` records at ``stride`` in the 1-D uint8 numpy array ``buf`` as strided views (u, v None: mono)."""
        h, w = self.header.height, self.header.width
        ch, cw = self.header.chroma_shape
        view = lambda off, r, c: np.lib.stride_tricks.as_strided(buf[off:], shape=(n, r, c), strides=(stride, c, 1), writeable=False)
        y = view(line, h, w)
        if self.chroma == "mono":
            return y, None, None
        return y, view(line + h * w, ch, cw), view(line + h * w + ch * cw, ch, cw)

    def planes(self, a, b):
        """Views (y (n, H, W), u, v (n, CH, CW); None for mono) of frames [a, b) in the memory-mapped file; [a, b) one of ``runs``."""
        buf, line, stride = self.records(a, b)
        return self.plane_views(buf, b - a, line, stride)

    def window(self, a, b, top, left, h, w):
        """Frames [a, b) (any range: it may cross ``runs``), luma crop [top, top + h) x [left, left + w) inside the frame -> the window
        (y (n, h, w), u, v) of the module docstring, uint8 copies of fixed shapes (window_chroma_shape; None for mono): plane bytes only,
        no colour arithmetic."""
        t, fh, fw, _ = self.shape
        if not 0 <= a <= b <= t:
            raise ValueError(f"{self.path}: frames [{a}, {b}) of {t}")
        if h < 1 or w < 1 or top < 0 or left < 0 or top + h > fh or left + w > fw:
            raise ValueError(f"{self.path}: the crop {h}x{w} at ({top}, {left}) does not lie inside frames of {fh}x{fw}")
        n = b - a
        y = np.empty((n, h, w), dtype=np.uint8)
        if self.chroma == "mono":
            u = v = None
        else:
            u, v = (np.empty((n,) + window_chroma_shape(h, w, self.chroma), dtype=np.uint8) for _ in range(2))
        if self.chroma == "420":
            ch, cw = self.header.chroma_shape
            rows = np.clip((top >> 1) - 1 + np.arange(u.shape[1]), 0, ch - 1)
            cols = np.clip((left >> 1) - 1 + np.arange(u.shape[2]), 0, cw - 1)
            rs, cs = slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1)
            rows, cols = (rows - rows[0])[:, None], (cols - cols[0])[None, :]
        for s, e in self.runs(a, b):
            py, pu, pv = self.planes(s, e)
            y[s - a:e - a] = py[:, top:top + h, left:left + w]
            if self.chroma == "444":
                u[s - a:e - a] = pu[:, top:top + h, left:left + w]
                v[s - a:e - a] = pv[:, top:top + h, left:left + w]
            elif self.chroma == "420":
                u[s - a:e - a] = pu[:, rs, cs][:, rows, cols]
                v[s - a:e - a] = pv[:, rs, cs][:, rows, cols]
        return y, u, v

    def __getitem__(self, key):
        if isinstance(key, (int, np.integer)):
            i = int(key) + (self.shape[0] if key < 0 else 0)
            if not 0 <= i < self.shape[0]:
                raise IndexError(f"{self.path}: frame {int(key)} of {self.shape[0]}")
            return self[i:i + 1][0]
        if not isinstance(key, slice):
            raise TypeError(f"{self.path}: a Y4MClip is indexed by a frame or a slice of frames")
        a, b, step = key.indices(self.shape[0])
        if step != 1:
            raise ValueError(f"{self.path}: frame slices have step 1")
        out = np.empty((max(b - a, 0),) + self.shape[1:], dtype=np.uint8)
        for s, e in self.runs(a, b):
            out[s - a:e - a] = yuv_to_rgb_reference(*self.planes(s, e), self.chroma, self.siting, self.matrix, self.full)
        return out


def _fps(fps):
    if isinstance(fps, str):
        n, _, d = fps.partition(":")
        return int(n), int(d or 1)
    if isinstance(fps, (tuple, list)):
        return int(fps[0]), int(fps[1])
    from fractions import Fraction
    f = Fraction(fps).limit_denominator(1001)
    return f.numerator, f.denominator


def write(path, rgb_or_planes, fps=(30, 1), chroma="420", matrix="bt601", full=False):
    """Write a .y4m file: ``rgb_or_planes`` uint8 RGB (T, H, W, 3), converted by rgb_to_yuv_reference, or planes (y, u, v) of the
    ``chroma`` form written as they are (u, v None for "mono").  4:2:0 is tagged C420jpeg; the header carries Ip and
    XCOLORRANGE=FULL / XCOLORRANGE=LIMITED.  ``fps``: (n, d), "n:d" or a number."""
    if chroma not in _WRITE_TAGS:
        raise ValueError(f"chroma {chroma!r}: one of {CHROMAS}")
    if isinstance(rgb_or_planes, (tuple, list)):
        y, u, v = _check_planes(*rgb_or_planes, chroma)
    else:
        y, u, v = rgb_to_yuv_reference(rgb_or_planes, chroma, matrix, full)
    t, h, w = y.shape
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"{path}: frames of {h}x{w}: sides 1 .. {MAX_SIDE}")
    n, d = _fps(fps)
    head = f"YUV4MPEG2 W{w} H{h} F{n}:{d} Ip C{_WRITE_TAGS[chroma]} XCOLORRANGE={'FULL' if full else 'LIMITED'}\n".encode("ascii")
    with open(path, "wb") as fh:
        fh.write(head)
        for i in range(t):
            fh.write(b"FRAME\n")
            fh.write(np.ascontiguousarray(y[i]).tobytes())
            if u is not None:
                fh.write(np.ascontiguousarray(u[i]).tobytes())
                fh.write(np.ascontiguousarray(v[i]).tobytes())
