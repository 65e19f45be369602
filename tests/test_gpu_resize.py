"""GPU: the crop + resize kernel (csrc/resize.hip) against its written specification (data.resize_reference_u8) and the host path
(data._resize_u8) of the cropped clip, byte for byte; device_centre_square and the run-by-run upload; a captured launch; the refusals;
``infer encode|eval --device-resize`` against the same commands without the flag."""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SMALL = 64

# name -> (clip shape (n, H, W, C), (top, left, crop_h, crop_w), (out_h, out_w))
CASES = {
    "centre_odd_left": ((3, 45, 80, 3), (0, 17, 45, 45), (32, 32)),            # the centre square of 45 x 80: left offset 17
    "ties_2x": ((2, 64, 64, 3), (0, 0, 64, 64), (32, 32)),                     # exact 2x: a quarter of the values end in .5
    "upscale": ((2, 20, 12, 3), (4, 0, 12, 12), (32, 32)),                     # the centre square of 20 x 12, edge clamp on both sides
    "crop_24x40": ((1, 48, 64, 3), (3, 5, 37, 53), (24, 40)),
    "crop_23x37": ((1, 48, 64, 3), (3, 5, 37, 53), (23, 37)),                  # rows of 111 bytes: no multiple of 4
    "one_channel": ((2, 33, 33, 1), (0, 0, 33, 33), (32, 32)),
    "two_channels": ((1, 9, 11, 2), (1, 2, 7, 8), (7, 5)),                     # rows of 10 bytes
    "four_channels": ((2, 21, 35, 4), (1, 2, 19, 30), (16, 27)),
    "identity": ((2, 32, 32, 3), (0, 0, 32, 32), (32, 32)),
    "wide_row": ((1, 10, 400, 3), (0, 3, 10, 390), (9, 350)),                  # rows of 1050 bytes: two workgroups across, a 2-byte tail
    "production": ((1, 720, 1280, 3), (0, 280, 720, 720), (256, 256)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(clip uint8 numpy, reference bytes) of a case; computed once, shared and left unchanged."""
    from video_vae_amd import data as D
    shape, (top, left, ch, cw), (oh, ow) = CASES[name]
    clip = np.random.default_rng(sorted(CASES).index(name)).integers(0, 256, size=shape, dtype=np.uint8)
    crop = np.ascontiguousarray(clip[:, top:top + ch, left:left + cw])
    want = D.resize_reference_u8(crop, oh, ow)
    host = D._resize_u8(crop, oh, ow)
    assert np.array_equal(want, host), name                                   # the specification is the host path
    clip.setflags(write=False)
    want.setflags(write=False)
    return clip, want


def _dev_clip(name, dev):
    return torch.from_numpy(np.array(_case(name)[0])).to(dev)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_reference_and_host_bytewise(dev, name):
    from video_vae_amd import ops
    _, crop, (oh, ow) = CASES[name]
    clip, want = _case(name)
    x = _dev_clip(name, dev)
    got = ops.crop_resize_u8(x, *crop, oh, ow)
    again = ops.crop_resize_u8(x, *crop, oh, ow)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    bad = int((got.cpu().numpy() != want).sum())
    print(f"{name}: {bad} of {want.size} bytes differ")
    assert bad == 0
    assert torch.equal(got, again)


@pytest.mark.parametrize("offset", [0, 5])
def test_rows_of_111_bytes_touch_nothing_outside_the_result(dev, offset):
    """dst is a view into a larger poisoned buffer (4-byte aligned, and not): the bytes before the first and after the last row stay."""
    from video_vae_amd import ops
    name = "crop_23x37"
    _, crop, (oh, ow) = CASES[name]
    _, want = _case(name)
    n = want.size
    for poison in (0xA5, 0x5A):
        buf = torch.full((n + 64,), poison, dtype=torch.uint8, device=dev)
        out = buf[offset:offset + n].view(want.shape)
        res = ops.crop_resize_u8(_dev_clip(name, dev), *crop, oh, ow, out=out)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert np.array_equal(host[offset:offset + n].reshape(want.shape), want)
        assert (host[:offset] == poison).all() and (host[offset + n:] == poison).all()


def test_two_frames_of_odd_rows_leave_the_poison_between_views(dev):
    """Two frames resized one by one into views of one buffer with a gap after each: every frame's last row ends where it must."""
    from video_vae_amd import ops
    shape, crop, (oh, ow) = (2, 48, 64, 3), (3, 5, 37, 53), (23, 37)
    from video_vae_amd import data as D
    clip = np.random.default_rng(77).integers(0, 256, size=shape, dtype=np.uint8)
    want = D.resize_reference_u8(np.ascontiguousarray(clip[:, 3:40, 5:58]), oh, ow)
    per = oh * ow * 3
    buf = torch.full((2 * (per + 7),), 0xEE, dtype=torch.uint8, device=dev)
    x = torch.from_numpy(clip).to(dev)
    for f in range(2):
        ops.crop_resize_u8(x[f:f + 1], *crop, oh, ow, out=buf[f * (per + 7):f * (per + 7) + per].view(1, oh, ow, 3))
    host = buf.cpu().numpy().reshape(2, per + 7)
    assert np.array_equal(host[:, :per].reshape(want.shape), want) and (host[:, per:] == 0xEE).all()


@pytest.mark.parametrize("name", ["centre_odd_left", "upscale", "production"])
def test_device_centre_square_equals_infer_centre_square(dev, name):
    from video_vae_amd import data as D
    from video_vae_amd.infer import centre_square
    shape, crop, (oh, ow) = CASES[name]
    assert D.centre_square_crop(shape[1], shape[2]) == (crop[0], crop[1], crop[2]) and crop[2] == crop[3] and oh == ow
    clip, want = _case(name)
    got = D.device_centre_square(_dev_clip(name, dev), oh)
    assert np.array_equal(got.cpu().numpy(), want)
    if name != "production":                                                  # the host path once more, through infer's own function
        assert np.array_equal(centre_square(np.array(clip), oh), want)


def test_upload_in_runs_of_one_frame_equals_one_shot(dev):
    from video_vae_amd import data as D
    clip, want = _case("centre_odd_left")
    one = D.upload_centre_square(clip, 32, dev)
    runs = D.upload_centre_square(clip, 32, dev, run_bytes=1)                 # less than a frame: runs of one frame
    assert one.shape == (3, 32, 32, 3) and torch.equal(one, runs) and np.array_equal(one.cpu().numpy(), want)
    two = D.upload_centre_square(clip, 32, dev, run_bytes=2 * 45 * 80 * 3)    # runs of two frames, the last one short
    assert torch.equal(one, two)


def test_captured_launch_replays_on_new_bytes(dev):
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    name = "crop_23x37"
    shape, crop, (oh, ow) = CASES[name]
    x = _dev_clip(name, dev)
    out = torch.empty((shape[0], oh, ow, shape[3]), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.crop_resize_u8(x, *crop, oh, ow, out=out)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.crop_resize_u8(x, *crop, oh, ow, out=out)
    census = graph_node_census(graph)
    assert census is None or census.get("memset", 0) == 0, census
    assert census is None or census.get("kernel", 1) == 1, census
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        new = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev)
        eager = ops.crop_resize_u8(new, *crop, oh, ow)
        x.copy_(new)
        out.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_refusals_raise_before_any_launch(dev):
    from video_vae_amd import ops
    x = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=dev)
    sentinel = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8, device=dev)
    bad = [dict(frames=x.float()), dict(frames=x.cpu()), dict(frames=x[0]),
           dict(top=9), dict(left=9), dict(top=-1), dict(left=-1), dict(crop_h=17), dict(crop_w=17),        # a crop outside the frame
           dict(crop_h=0), dict(out_h=0, out=None), dict(out_w=16385, out=None),                            # extents the kernel refuses
           dict(frames=torch.zeros((1, 16, 16, 5), dtype=torch.uint8, device=dev), out=None),
           dict(out=sentinel[:, :4]), dict(out=sentinel.float()), dict(out=sentinel.cpu())]
    for kw in bad:
        a = dict(frames=x, top=0, left=0, crop_h=8, crop_w=8, out_h=8, out_w=8, out=sentinel)
        a.update(kw)
        with pytest.raises(ops.VvaeError):
            ops.crop_resize_u8(**a)
    torch.cuda.synchronize()
    assert (sentinel == 7).all()
    from video_vae_amd._lib import lib
    import ctypes
    p = ctypes.c_void_p(x.data_ptr())
    q = ctypes.c_void_p(sentinel.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((1, 16, 16, 3, 9, 0, 8, 8, 8, 8), (1, 16, 16, 3, 0, 9, 8, 8, 8, 8), (1, 16, 16, 3, -1, 0, 8, 8, 8, 8), (0, 16, 16, 3, 0, 0, 8, 8, 8, 8)):
        assert lib().vvae_crop_resize_u8(p, q, *args, st) == 1001, args        # the launcher's own check
    assert lib().vvae_crop_resize_u8(None, q, 1, 16, 16, 3, 0, 0, 8, 8, 8, 8, st) == 1001
    torch.cuda.synchronize()
    assert (sentinel == 7).all()


# ------------------------------------------------------------------------------------------------ command line
def _small(seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    return rl_model.VideoVAE(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _run(args):
    """The command in this process (infer.main is what ``python -m video_vae_amd.infer`` calls): twelve runs without twelve interpreters."""
    from video_vae_amd import infer
    infer.main([str(a) for a in args])


def _common(tmp_path, data):
    return ["--model_path", str(tmp_path / "ckpt"), "--data", str(data), "--size", str(SMALL), "--frames", "4", "--batch", "4",
            "--small", "--threshold"]


def _scene(rng, frames, hw, lo, hi):
    """Frames of one 4-colour palette drawn from [lo, hi), the same proportions in new places in every frame: one histogram per scene."""
    pal = rng.integers(lo, hi, size=(4, 3))
    return np.stack([pal[rng.permutation(np.arange(hw[0] * hw[1]) % 4).reshape(hw)] for _ in range(frames)]).astype(np.uint8)


def _clips():
    """40 x 56 (a downscale of the 40 x 40 centre, left offset 8), 10 frames in two scenes of distinct colour; 24 x 30 (an upscale), 6
    frames; 40 x 56 with 3 frames: shorter than a window."""
    rng = np.random.default_rng(4)
    return {"wide": np.concatenate([_scene(rng, 6, (40, 56), 0, 70), _scene(rng, 4, (40, 56), 180, 256)]),
            "low": _scene(rng, 6, (24, 30), 0, 256), "short": _scene(rng, 3, (40, 56), 0, 256)}


def _data(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    for name, clip in _clips().items():
        np.save(data / f"{name}.npy", clip)
    return data


MODES = {"plain": [], "overlap": ["--temporal-overlap", "2"], "scenes": ["--scene-cuts", "--temporal-overlap", "2"]}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_device_resize_writes_the_host_path_s_results(dev, tmp_path, mode):
    from video_vae_amd import model_loader
    data = _data(tmp_path)
    model_loader.save_checkpoint(_small(9), None, str(tmp_path / "ckpt"))
    extra = MODES[mode]
    res = {}
    for tag, flag in (("host", []), ("device", ["--device-resize"])):
        _run(["encode"] + _common(tmp_path, data) + extra + flag + ["--out", str(tmp_path / f"lat_{tag}")])
        _run(["eval"] + _common(tmp_path, data) + extra + flag + ["--per-frame", "--temporal-metrics", "--out", str(tmp_path / f"{tag}.json")])
        res[tag] = json.loads((tmp_path / f"{tag}.json").read_text())
    for name in ("wide", "low", "short"):
        with np.load(tmp_path / "lat_host" / f"{name}.npz") as a, np.load(tmp_path / "lat_device" / f"{name}.npz") as b:
            assert sorted(a.files) == sorted(b.files)
            for k in a.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
            if mode == "scenes":
                assert a["scene_cuts"].tolist() == ([6] if name == "wide" else [])
    assert res["host"]["config"].pop("resize") == "host" and res["device"]["config"].pop("resize") == "device"
    assert res["host"] == res["device"]
    assert res["host"]["dataset"]["frames"] == 19 and len(res["host"]["clips"]) == 3
