"""GPU: the window kernel (csrc/yuv_window.hip: vvae_yuv_window_resize_norm, ops.yuv_window_resize_norm) against
y4m.window_to_rgb_reference -> data.resize_reference_u8 -> / 255, bit for bit in fp32 and bf16, over every chroma form, siting, matrix,
range and parity; the frame -> clip map; past 65 535 frames; an out= view in a poisoned buffer; a captured launch; the refusals;
DevicePrefetcher(yuv=...) against the host-converting loader; ``train --device-yuv`` against ``train`` without it."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
FORMS = {"420_centre": ("420", "centre"), "420_mpeg2": ("420", "mpeg2"), "444": ("444", "centre"), "mono": ("mono", "centre")}
# one clip per (top & 1, left & 1, full range): a launch of 8 one-frame clips covers every parity in both ranges
PARAMS = [(py, px, full, 0) for py in (0, 1) for px in (0, 1) for full in (0, 1)]

# name -> ((h, w) of the luma crop, (out_h, out_w)); "span*": the width is taken from the kernel's exported constant (see _size)
SIZES = {
    "1x1": ((1, 1), (1, 1)), "2x3": ((2, 3), (2, 3)), "2x3_to_1x1": ((2, 3), (1, 1)), "5x7": ((5, 7), (5, 7)), "5x7_to_1x1": ((5, 7), (1, 1)),
    "5x7_up": ((5, 7), (9, 12)),                                          # upscale: edge taps with x1 = x0 and a weight on them
    "36": ((36, 36), (36, 36)), "36_to_18": ((36, 36), (18, 18)), "36_to_32": ((36, 36), (32, 32)),
    "36_to_18x36": ((36, 36), (18, 36)), "36_to_36x18": ((36, 36), (36, 18)),      # one axis copied, the other halved
    "21x53": ((21, 53), (21, 53)), "21x53_to_8x8": ((21, 53), (8, 8)), "21x53_to_1x1": ((21, 53), (1, 1)), "22x54_to_11x27": ((22, 54), (11, 27)),
    "span_copy-1": "copy", "span_copy+0": "copy", "span_copy+1": "copy",
    "span_half-1": "half", "span_half+0": "half", "span_half+1": "half",
    "span_any-1": "any", "span_any+0": "any", "span_any+1": "any",
}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _size(name):
    """((h, w), (out_h, out_w)) of a case; the span cases put out_w just below, at and just past one workgroup's pixels of a row."""
    from video_vae_amd import ops
    spec = SIZES[name]
    if not isinstance(spec, str):
        return spec
    delta = int(name[-2:])
    if spec == "copy":
        w = ops.yuv_window_span() + delta
        return (3, w), (3, w)
    if spec == "half":
        ow = ops.yuv_window_span() + delta
        return (4, 2 * ow), (2, ow)
    ow = ops.yuv_window_span() + delta
    return (3, ow + 7), (2, ow)


def _windows(rng, n, h, w, chroma):
    from video_vae_amd import y4m
    y = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    if chroma == "mono":
        return y, None, None
    cs = (n,) + y4m.window_chroma_shape(h, w, chroma)
    return y, rng.integers(0, 256, size=cs, dtype=np.uint8), rng.integers(0, 256, size=cs, dtype=np.uint8)


def _reference(win, params, frames_per_clip, chroma, siting, matrix, out_h, out_w):
    """fp32 (n, out_h, out_w, 3): window_to_rgb_reference -> resize_reference_u8 -> / 255, every frame with its clip's params row."""
    from video_vae_amd import data as D, y4m
    y, u, v = win
    n = y.shape[0]
    out = np.empty((n, out_h, out_w, 3), dtype=np.float32)
    rows = np.arange(n) // frames_per_clip
    for row in sorted(set(map(tuple, np.asarray(params)[:, :3].tolist()))):
        sel = np.flatnonzero((np.asarray(params)[rows, :3] == row).all(axis=1))
        rgb = y4m.window_to_rgb_reference(y[sel], None if u is None else u[sel], None if v is None else v[sel], row[:2], chroma, siting, matrix,
                                          bool(row[2]))
        out[sel] = D.resize_reference_u8(rgb, out_h, out_w).astype(np.float32) / np.float32(255)
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=None)
def _case(form, name, matrix):
    """(windows, params, fp32 reference) of a case: computed once, shared and left unchanged."""
    chroma, siting = FORMS[form]
    (h, w), (oh, ow) = _size(name)
    rng = np.random.default_rng(sorted(SIZES).index(name) * 8 + sorted(FORMS).index(form))
    win = _windows(rng, len(PARAMS), h, w, chroma)
    params = np.array(PARAMS, dtype=np.int32)
    return win, params, _reference(win, params, 1, chroma, siting, matrix, oh, ow)


def _dev(win, dev):
    return tuple(None if p is None else torch.from_numpy(np.array(p)).to(dev) for p in win)


@pytest.mark.parametrize("name", sorted(SIZES))
@pytest.mark.parametrize("form", sorted(FORMS))
def test_kernel_equals_reference_bitwise(dev, form, name):
    from video_vae_amd import ops
    chroma, siting = FORMS[form]
    (h, w), (oh, ow) = _size(name)
    for matrix in ("bt601", "bt709"):
        win, params, want = _case(form, name, matrix)
        y, u, v = _dev(win, dev)
        p = torch.from_numpy(params).to(dev)
        for dt, dtype in DTYPES.items():
            got = ops.yuv_window_resize_norm(y, u, v, p, 1, chroma, siting, matrix, oh, ow, dtype=dtype)
            again = ops.yuv_window_resize_norm(y, u, v, p, 1, chroma, siting, matrix, oh, ow, dtype=dtype)
            torch.cuda.synchronize()
            ref = want.to(dtype)
            assert got.dtype == dtype and tuple(got.shape) == (len(PARAMS), oh, ow, 3)
            bad = (_bits(got.cpu()) != _bits(ref)).flatten(1).sum(1).tolist()
            print(f"{form} {name} {h}x{w}->{oh}x{ow} {matrix} {dt}: differing elements per (py, px, full) clip: {bad}")
            assert not any(bad)
            assert torch.equal(_bits(got), _bits(again))


def test_equal_extents_are_the_conversion_divided(dev):
    """crop_size == size: exactly vvae_yuv_to_rgb_u8's bytes of the same planes, each divided by 255 (the two-launch route's values)."""
    from video_vae_amd import ops, y4m
    rng = np.random.default_rng(21)
    H, W, top, left, h, w = 30, 44, 3, 5, 20, 32
    y = rng.integers(0, 256, size=(2, H, W), dtype=np.uint8)
    u, v = (rng.integers(0, 256, size=(2, H // 2, W // 2), dtype=np.uint8) for _ in range(2))
    rows = np.clip((top >> 1) - 1 + np.arange(h // 2 + 3), 0, H // 2 - 1)[:, None]
    cols = np.clip((left >> 1) - 1 + np.arange(w // 2 + 3), 0, W // 2 - 1)[None, :]
    win = (np.ascontiguousarray(y[:, top:top + h, left:left + w]), np.ascontiguousarray(u[:, rows, cols]), np.ascontiguousarray(v[:, rows, cols]))
    rgb = ops.yuv_to_rgb_u8(*_dev((y, u, v), dev))
    two = ops.crop_resize_norm(rgb, top, left, h, w, h, w, dtype=torch.bfloat16)
    p = torch.tensor([[top & 1, left & 1, 0, 0]], dtype=torch.int32, device=dev)
    one = ops.yuv_window_resize_norm(*_dev(win, dev), p, 2, out_h=h, out_w=w, dtype=torch.bfloat16)
    assert torch.equal(_bits(one), _bits(two))
    assert np.array_equal(y4m.window_to_rgb_reference(*win, (top & 1, left & 1)), rgb[:, top:top + h, left:left + w].cpu().numpy())


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_frames_take_their_clip_s_params(dev, dt):
    """Three clips x two frames with three different rows, and n = 5: the last clip is short.  A wrong frame -> clip map changes bytes."""
    from video_vae_amd import ops
    rng = np.random.default_rng(31)
    win = _windows(rng, 5, 9, 14, "420")
    params = np.array([(1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 0, 0)], dtype=np.int32)
    want = _reference(win, params, 2, "420", "centre", "bt709", 6, 7).to(DTYPES[dt])
    wrong = _reference(win, params[[0, 0, 1]], 2, "420", "centre", "bt709", 6, 7).to(DTYPES[dt])
    assert all(not torch.equal(_bits(want[i]), _bits(wrong[i])) for i in (2, 3, 4))
    got = ops.yuv_window_resize_norm(*_dev(win, dev), torch.from_numpy(params).to(dev), 2, "420", "centre", "bt709", 6, 7, dtype=DTYPES[dt])
    assert torch.equal(_bits(got.cpu()), _bits(want))


def test_65537_frames_of_2x2(dev):
    from video_vae_amd import ops
    n = 65537
    rng = np.random.default_rng(41)
    win = _windows(rng, n, 2, 2, "420")
    params = np.concatenate([rng.integers(0, 2, size=(n, 3)), np.zeros((n, 1), dtype=np.int64)], axis=1).astype(np.int32)
    want = _reference(win, params, 1, "420", "centre", "bt601", 2, 2)
    got = ops.yuv_window_resize_norm(*_dev(win, dev), torch.from_numpy(params).to(dev), 1, out_h=2, out_w=2)
    bad = (_bits(got.cpu()) != _bits(want)).flatten(1).any(1)
    print(f"frames that differ: {int(bad.sum())} of {n}; the first: {bad.nonzero().flatten()[:4].tolist()}")
    assert not bad.any()


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ["5x7", "36_to_18", "21x53_to_8x8"])
def test_unaligned_out_view_and_its_guards(dev, name, dt):
    """out= starts one element past 8 guard elements of an aligned buffer: no vector store is aligned.  The guards keep their poison."""
    from video_vae_amd import ops
    (h, w), (oh, ow) = _size(name)
    win, params, want = _case("420_centre", name, "bt601")
    want = want.to(DTYPES[dt])
    n = want.numel()
    for poison in (-7.0, 3.0):
        buf = torch.full((9 + n + 8,), poison, dtype=DTYPES[dt], device=dev)
        out = buf[9:9 + n].view(want.shape)
        res = ops.yuv_window_resize_norm(*_dev(win, dev), torch.from_numpy(params).to(dev), 1, out_h=oh, out_w=ow, dtype=DTYPES[dt], out=out)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        host = buf.cpu()
        assert torch.equal(_bits(host[9:9 + n].view(want.shape)), _bits(want))
        assert (host[:9] == poison).all() and (host[9 + n:] == poison).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_captured_launch_replays_on_new_bytes(dev, dt):
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    (h, w), (oh, ow) = _size("36_to_18")
    win, params, _ = _case("420_centre", "36_to_18", "bt601")
    y, u, v = _dev(win, dev)
    p = torch.from_numpy(params).to(dev)
    out = torch.empty((len(PARAMS), oh, ow, 3), dtype=DTYPES[dt], device=dev)
    run = lambda dst: ops.yuv_window_resize_norm(y, u, v, p, 1, out_h=oh, out_w=ow, dtype=DTYPES[dt], out=dst)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(out)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run(out)
    census = graph_node_census(graph)
    assert census is None or census.get("memset", 0) == 0, census
    assert census is None or census.get("kernel", 1) == 1, census
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        new = [torch.randint(0, 256, t.shape, generator=g, dtype=torch.uint8).to(dev) for t in (y, u, v)]
        eager = ops.yuv_window_resize_norm(*new, p, 1, out_h=oh, out_w=ow, dtype=DTYPES[dt])
        for t, src in zip((y, u, v), new):
            t.copy_(src)
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager))


def test_refusals_launch_nothing(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import lib
    y = torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)
    c = torch.zeros((2, 7, 7), dtype=torch.uint8, device=dev)
    p = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    sentinel = torch.full((2, 4, 4, 3), 7.0, dtype=torch.float32, device=dev)
    wide = torch.zeros((2, 7, 14), dtype=torch.uint8, device=dev)
    bad = [dict(y=y.cpu()), dict(y=y.float()), dict(y=y[0]), dict(u=c.cpu()), dict(v=c[:, :6]), dict(u=None), dict(u=wide[:, :, ::2]),
           dict(clip_params=p.cpu()), dict(clip_params=p.long()), dict(clip_params=p[:, :3]), dict(clip_params=torch.zeros((2, 4), dtype=torch.int32, device=dev)),
           dict(frames_per_clip=1), dict(frames_per_clip=0), dict(chroma="422"), dict(siting="left"), dict(matrix="bt2020"),
           dict(chroma="444"), dict(dtype=torch.float16, out=None), dict(out_h=0, out=None), dict(out_w=16385, out=None),
           dict(out=sentinel[:, :2]), dict(out=sentinel.to(torch.bfloat16)), dict(out=sentinel.cpu())]
    for kw in bad:
        a = dict(y=y, u=c, v=c, clip_params=p, frames_per_clip=2, chroma="420", siting="centre", matrix="bt601", out_h=4, out_w=4,
                 dtype=torch.float32, out=sentinel)
        a.update(kw)
        with pytest.raises(ops.VvaeError):
            ops.yuv_window_resize_norm(**a)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = lib().vvae_yuv_window_resize_norm
    for bf16 in (0, 1):
        for args in ((0, 2, 8, 8, 0, 0, 0, 4, 4), (-1, 2, 8, 8, 0, 0, 0, 4, 4), (2, 0, 8, 8, 0, 0, 0, 4, 4), (2, 2, 0, 8, 0, 0, 0, 4, 4),
                     (2, 2, 8, 16385, 0, 0, 0, 4, 4), (2, 2, 8, 8, 3, 0, 0, 4, 4), (2, 2, 8, 8, 0, 2, 0, 4, 4), (2, 2, 8, 8, 0, 0, 2, 4, 4),
                     (2, 2, 8, 8, 0, 0, 0, 0, 4), (2, 2, 8, 8, 0, 0, 0, 4, 16385)):
            assert fn(P(y), P(c), P(c), P(p), P(sentinel), bf16, *args, st) == 1001, args
        assert fn(None, P(c), P(c), P(p), P(sentinel), bf16, 2, 2, 8, 8, 0, 0, 0, 4, 4, st) == 1001
        assert fn(P(y), None, P(c), P(p), P(sentinel), bf16, 2, 2, 8, 8, 0, 0, 0, 4, 4, st) == 1001
        assert fn(P(y), P(c), P(c), None, P(sentinel), bf16, 2, 2, 8, 8, 0, 0, 0, 4, 4, st) == 1001
        assert fn(P(y), P(c), P(c), P(p), None, bf16, 2, 2, 8, 8, 0, 0, 0, 4, 4, st) == 1001
    torch.cuda.synchronize()
    assert (sentinel == 7).all()


# ------------------------------------------------------------------------------------------------ the loader
def _folder(base, height, width, n):
    """``n`` 4:2:0 clips of 8 frames (every third one short) and a truncated file: the zero fallback with an all-ones mask."""
    from video_vae_amd import data as D
    d = D.write_synthetic_clips(str(base), n, 8, height, width, seed=4, ext=".y4m")
    raw = open(os.path.join(d, "clip0001.y4m"), "rb").read()
    open(os.path.join(d, "cut.y4m"), "wb").write(raw[:len(raw) - 100])
    return str(base)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_prefetcher_device_yuv_equals_host_conversion(dev, tmp_path, capfd, dt):
    from video_vae_amd import data as D
    base = _folder(tmp_path, 40, 48, 6)
    conf = {"matrix": "bt709", "range": "header"}

    def loader(**kw):
        return D.create_batched_dataloader(base, batch_size=2, max_frames=8, resize=(32, 32), crop_size=36, shuffle=True, seed=3,
                                           num_workers=2, as_uint8=True, y4m=conf, **kw)
    want = [{k: v.clone() for k, v in b.items()} for b in D.DevicePrefetcher(loader(), dev, DTYPES[dt])]
    planes = loader(device_yuv=True)
    got = [{k: v.clone() for k, v in b.items()} for b in D.DevicePrefetcher(planes, dev, DTYPES[dt], resize=(32, 32), yuv=planes.yuv)]
    torch.cuda.synchronize()
    assert len(got) == len(want) == 4                                     # 7 clips in batches of 2, the last one single
    short = fallback = 0
    for a, b in zip(got, want):
        assert sorted(a) == ["mask", "video"]
        assert a["video"].dtype == DTYPES[dt] and a["video"].shape == b["video"].shape and a["video"].shape[1:] == (8, 32, 32, 3)
        assert torch.equal(_bits(a["video"]), _bits(b["video"]))
        assert a["mask"].dtype == torch.float32 and torch.equal(a["mask"], b["mask"])
        short += int((b["mask"].sum(1) < 8).sum())
        fallback += int((b["video"].flatten(1).abs().sum(1) == 0).sum())
    assert short == 2 and fallback == 1
    capfd.readouterr()


def test_prefetcher_yuv_refuses_a_batch_without_planes(dev):
    import gc
    from video_vae_amd import data as D
    p = D.DevicePrefetcher([{"video": torch.zeros((1, 2, 8, 8, 3), dtype=torch.uint8), "mask": torch.ones((1, 2))}], dev, resize=(4, 4),
                           yuv={"chroma": "420", "siting": "centre", "matrix": "bt601"})
    with pytest.raises(ValueError, match="plane batches"):
        next(p)
    p.err = None                                                          # the stored traceback holds device objects in a cycle
    del p
    gc.collect()


def _train(args):
    """One ``python -m video_vae_amd.train`` run in a fresh child with its own time limit -> its loss lines, the wall clock cut out."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-m", "video_vae_amd.train"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return [re.sub(r"time = [0-9.]+, ", "", l) for l in r.stdout.splitlines() if l.startswith("Epoch ")]


def test_train_device_yuv_prints_the_host_conversion_s_losses(dev, tmp_path):
    """The replayed step is a pure function of its inputs, so equal batches must give equal text."""
    torch.cuda.empty_cache()
    base = _folder(tmp_path, 56, 64, 8)                                       # 9 clips: 4 batches of 2
    common = ["--small", "--size", "32", "--crop_size", "48", "--per_device_batch_size", "2", "--max_frames", "8", "--steps", "4",
              "--log_every", "1", "--y4m-matrix", "bt709", "--data", base]
    host = _train(common)
    device = _train(common + ["--device-yuv"])
    print("\n".join(host))
    assert len(host) == 4 and all("Loss = " in l and "nan" not in l.lower() for l in host), host
    assert "mode = hipgraph" in host[-1]
    assert device == host
