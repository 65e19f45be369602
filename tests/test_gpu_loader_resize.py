"""GPU: the normalising output of the crop + resize kernel (csrc/resize.hip: vvae_crop_resize_norm, ops.crop_resize_norm) against
data.resize_reference_u8 of the crop divided by 255, bit for bit in fp32 and bf16; an unaligned destination; a captured launch; the
launcher's refusals; DevicePrefetcher(resize=...) against the host-resizing loader; ``train --device-resize`` against ``train`` without it."""
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

# name -> (frames shape (n, H, W, C), (top, left, crop_h, crop_w), (out_h, out_w))
CASES = {
    "row_of_21": ((3, 17, 19, 3), (3, 2, 9, 13), (5, 7)),                      # 21 elements a row: the last thread of a row owns 1
    "36_to_32": ((2, 36, 36, 3), (0, 0, 36, 36), (32, 32)),                    # the tests' loader shape
    "64_to_32": ((2, 64, 64, 3), (0, 0, 64, 64), (32, 32)),                    # exact 2x: a quarter of the values are ties
    "upscale": ((2, 8, 8, 3), (0, 0, 8, 8), (16, 16)),
    "one_channel": ((2, 17, 19, 1), (3, 2, 9, 13), (5, 7)),                    # rows of 7
    "four_channels": ((2, 17, 19, 4), (3, 2, 9, 13), (5, 7)),
    "wide_row": ((1, 10, 400, 3), (0, 3, 10, 390), (9, 350)),                  # 1050 elements a row: two workgroups across, a tail of 2
}


def _bits(t):
    """A float tensor's bit patterns, for comparisons that tell -0 from 0 and never call two NaNs equal or unequal by accident."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(frames uint8 numpy, {dtype name: reference tensor}) of a case; computed once, shared and left unchanged."""
    from video_vae_amd import data as D
    shape, (top, left, ch, cw), (oh, ow) = CASES[name]
    frames = np.random.default_rng(100 + sorted(CASES).index(name)).integers(0, 256, size=shape, dtype=np.uint8)
    q = D.resize_reference_u8(np.ascontiguousarray(frames[:, top:top + ch, left:left + cw]), oh, ow)
    f32 = torch.from_numpy(q.astype(np.float32) / np.float32(255))
    frames.setflags(write=False)
    return frames, {"fp32": f32, "bf16": f32.to(torch.bfloat16)}


def _dev_frames(name, dev):
    return torch.from_numpy(np.array(_case(name)[0])).to(dev)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_all_256_bytes_divide_exactly(dev, dt):
    """Equal extents copy, so the output is q / 255 for every byte q there is: the division is proved over its whole domain."""
    from video_vae_amd import ops
    q = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    want = torch.from_numpy(q.astype(np.float32) / np.float32(255))
    if dt == "bf16":
        want = want.to(torch.bfloat16)
    got = ops.crop_resize_norm(torch.from_numpy(q).to(dev), 0, 0, 16, 16, 16, 16, dtype=DTYPES[dt])
    assert got.dtype == DTYPES[dt] and tuple(got.shape) == (1, 16, 16, 1)
    bad = (_bits(got.cpu()) != _bits(want)).flatten().nonzero().flatten().tolist()
    print(f"{dt}: bytes whose quotient differs: {bad}")
    assert not bad


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_reference_over_255_bitwise(dev, name, dt):
    from video_vae_amd import ops
    _, crop, (oh, ow) = CASES[name]
    want = _case(name)[1][dt]
    x = _dev_frames(name, dev)
    got = ops.crop_resize_norm(x, *crop, oh, ow, dtype=DTYPES[dt])
    again = ops.crop_resize_norm(x, *crop, oh, ow, dtype=DTYPES[dt])
    torch.cuda.synchronize()
    assert got.dtype == DTYPES[dt] and got.shape == want.shape
    bad = int((_bits(got.cpu()) != _bits(want)).sum())
    print(f"{name} {dt}: {bad} of {want.numel()} elements differ")
    assert bad == 0
    assert torch.equal(_bits(got), _bits(again))
    q = ops.crop_resize_u8(x, *crop, oh, ow)                                   # and it is the byte entry's q, divided
    assert torch.equal(_bits(torch.div(q.float(), torch.full((), 255.0, device=dev)).to(DTYPES[dt])), _bits(got))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ["row_of_21", "36_to_32"])
def test_unaligned_out_view_and_its_guards(dev, name, dt):
    """out= starts one element past 8 guard elements of an aligned buffer, so no vector store is aligned: every thread stores element by
    element (36_to_32: rows of 96, a multiple of 4; row_of_21: a row tail as well).  The guards on both sides keep their poison."""
    from video_vae_amd import ops
    _, crop, (oh, ow) = CASES[name]
    want = _case(name)[1][dt]
    n = want.numel()
    for poison in (-7.0, 3.0):
        buf = torch.full((9 + n + 8,), poison, dtype=DTYPES[dt], device=dev)
        assert buf.data_ptr() % 16 == 0
        out = buf[9:9 + n].view(want.shape)
        res = ops.crop_resize_norm(_dev_frames(name, dev), *crop, oh, ow, dtype=DTYPES[dt], out=out)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        host = buf.cpu()
        assert torch.equal(_bits(host[9:9 + n].view(want.shape)), _bits(want))
        assert (host[:9] == poison).all() and (host[9 + n:] == poison).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_captured_launch_replays_on_new_bytes(dev, dt):
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    name = "row_of_21"
    shape, crop, (oh, ow) = CASES[name]
    x = _dev_frames(name, dev)
    out = torch.empty((shape[0], oh, ow, shape[3]), dtype=DTYPES[dt], device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.crop_resize_norm(x, *crop, oh, ow, dtype=DTYPES[dt], out=out)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.crop_resize_norm(x, *crop, oh, ow, dtype=DTYPES[dt], out=out)
    census = graph_node_census(graph)
    assert census is None or census.get("memset", 0) == 0, census
    assert census is None or census.get("kernel", 1) == 1, census
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        new = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev)
        eager = ops.crop_resize_norm(new, *crop, oh, ow, dtype=DTYPES[dt])
        x.copy_(new)
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager))


def test_refusals_launch_nothing(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import lib
    x = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=dev)
    sentinel = torch.full((1, 8, 8, 3), 7.0, dtype=torch.float32, device=dev)
    bad = [dict(frames=x.float()), dict(frames=x.cpu()), dict(frames=x[0]), dict(dtype=torch.float16, out=None),
           dict(top=9), dict(left=-1), dict(crop_h=17), dict(crop_w=0), dict(out_h=0, out=None), dict(out_w=16385, out=None),
           dict(frames=torch.zeros((1, 16, 16, 5), dtype=torch.uint8, device=dev), out=None),
           dict(out=sentinel[:, :4]), dict(out=sentinel.to(torch.bfloat16)), dict(out=sentinel.cpu())]
    for kw in bad:
        a = dict(frames=x, top=0, left=0, crop_h=8, crop_w=8, out_h=8, out_w=8, out=sentinel)
        a.update(kw)
        with pytest.raises(ops.VvaeError):
            ops.crop_resize_norm(**a)
    p = ctypes.c_void_p(x.data_ptr())
    q = ctypes.c_void_p(sentinel.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = lib().vvae_crop_resize_norm
    for bf16 in (0, 1):
        for args in ((0, 16, 16, 3, 0, 0, 8, 8, 8, 8), (-1, 16, 16, 3, 0, 0, 8, 8, 8, 8),                      # n < 1
                     (1, 16, 16, 3, 9, 0, 8, 8, 8, 8), (1, 16, 16, 3, 0, 9, 8, 8, 8, 8), (1, 16, 16, 3, -1, 0, 8, 8, 8, 8),   # crop outside
                     (1, 16, 16, 5, 0, 0, 8, 8, 8, 8)):                                                           # C = 5
            assert fn(p, q, bf16, *args, st) == 1001, args
        assert fn(None, q, bf16, 1, 16, 16, 3, 0, 0, 8, 8, 8, 8, st) == 1001
        assert fn(p, None, bf16, 1, 16, 16, 3, 0, 0, 8, 8, 8, 8, st) == 1001
    torch.cuda.synchronize()
    assert (sentinel == 7).all()


# ------------------------------------------------------------------------------------------------ the loader
def _clips(base, height, width, n):
    """``n`` clips of 8 frames at height x width (every third one short) and one at half that size, which takes the host upscale."""
    from video_vae_amd import data as D
    d = D.write_synthetic_clips(str(base), n, 8, height, width)
    np.save(f"{d}/small.npy", np.random.default_rng(5).integers(0, 256, size=(8, height // 2, width // 2, 3), dtype=np.uint8))
    return str(base)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_prefetcher_device_resize_equals_host_resize(dev, tmp_path, dt):
    from video_vae_amd import data as D
    base = _clips(tmp_path, 40, 48, 6)

    def loader(**kw):
        return D.create_batched_dataloader(base, batch_size=2, max_frames=8, resize=(32, 32), crop_size=36, shuffle=True, seed=3,
                                           num_workers=2, as_uint8=True, **kw)
    want = [{k: v.clone() for k, v in b.items()} for b in D.DevicePrefetcher(loader(), dev, DTYPES[dt])]
    got = [{k: v.clone() for k, v in b.items()} for b in D.DevicePrefetcher(loader(device_resize=True), dev, DTYPES[dt], resize=(32, 32))]
    torch.cuda.synchronize()
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert a["video"].dtype == DTYPES[dt] and a["video"].shape == b["video"].shape and a["video"].shape[1:] == (8, 32, 32, 3)
        assert torch.equal(_bits(a["video"]), _bits(b["video"]))
        assert a["mask"].dtype == torch.float32 and torch.equal(a["mask"], b["mask"])


def test_prefetcher_resize_refuses_a_float_batch(dev):
    import gc
    from video_vae_amd import data as D
    p = D.DevicePrefetcher([{"video": np.zeros((1, 2, 8, 8, 3), np.float32), "mask": np.ones((1, 2), np.float32)}], dev, resize=(4, 4))
    with pytest.raises(ValueError, match="uint8"):
        next(p)
    # the stored exception's traceback holds the prefetcher's frames and they hold it: a cycle with device tensors, a stream and pinned
    # memory in it.  Left to the collector it can be collected in a loader worker forked later, which then calls the GPU runtime and dies
    p.err = None
    del p
    gc.collect()


def _train(args):
    """One ``python -m video_vae_amd.train`` run in a fresh child with its own time limit -> its loss lines, the wall clock cut out."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-m", "video_vae_amd.train"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return [re.sub(r"time = [0-9.]+, ", "", l) for l in r.stdout.splitlines() if l.startswith("Epoch ")]


def test_train_device_resize_prints_the_host_resize_s_losses(dev, tmp_path):
    """The replayed step is a pure function of its inputs, so equal batches must give equal text."""
    torch.cuda.empty_cache()
    base = _clips(tmp_path, 56, 64, 8)                                        # 9 clips: 4 batches of 2
    common = ["--small", "--size", "32", "--crop_size", "48", "--per_device_batch_size", "2", "--max_frames", "8", "--steps", "4",
              "--log_every", "1", "--data", base]
    host = _train(common)
    device = _train(common + ["--device-resize"])
    print("\n".join(host))
    assert len(host) == 4 and all("Loss = " in l and "nan" not in l.lower() for l in host), host
    assert "mode = hipgraph" in host[-1]
    assert device == host
