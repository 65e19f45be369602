"""CPU: the written specification of the bilinear uint8 resize (data.resize_reference_u8) against the host path it restates
(data._resize_u8, torch's interpolate), byte for byte and without tolerance; its rounding mode, pinned independently of torch; the library's
new symbols; the ``--device-resize`` flag of the parser."""
import numpy as np
import pytest
import torch

# (input h, w) -> (output h, w): down- and upscales by odd ratios, exact 2x (ties), non-square
EXTENTS = [((720, 720), (256, 256)), ((1080, 1080), (256, 256)), ((512, 512), (256, 256)), ((480, 480), (256, 256)),
           ((360, 360), (256, 256)), ((100, 100), (256, 256)), ((45, 45), (32, 32)), ((64, 64), (32, 32)), ((48, 48), (32, 32)),
           ((20, 20), (32, 32)), ((40, 56), (32, 32)), ((37, 53), (24, 40))]


def _clip(hw, channels=3, frames=2):
    return np.random.default_rng(0).integers(0, 256, size=(frames,) + tuple(hw) + (channels,), dtype=np.uint8)


@pytest.mark.parametrize("src,dst", EXTENTS)
def test_reference_equals_host_resize_bytewise(src, dst):
    from video_vae_amd import data as D
    clip = _clip(src)
    got = D.resize_reference_u8(clip, *dst)
    want = D._resize_u8(clip, *dst)
    assert got.dtype == np.uint8 and got.shape == (2,) + dst + (3,)
    assert int((got != want).sum()) == 0


def test_reference_equals_host_resize_smooth_frame_and_one_channel():
    from video_vae_amd import data as D
    y, x = np.mgrid[0:720, 0:720].astype(np.float64)
    smooth = np.stack([127.5 + 127.5 * np.sin(x / 37.0) * np.cos(y / 53.0), (x + y) * (255.0 / 1438.0), 255.0 * np.exp(-((x - 300) ** 2 + (y - 400) ** 2) / 9e4)],
                      axis=-1).round().astype(np.uint8)[None]
    assert int((D.resize_reference_u8(smooth, 256, 256) != D._resize_u8(smooth, 256, 256)).sum()) == 0
    one = _clip((33, 47), channels=1)
    got = D.resize_reference_u8(one, 32, 24)
    assert got.shape == (2, 32, 24, 1) and int((got != D._resize_u8(one, 32, 24)).sum()) == 0


def test_equal_extents_return_the_input_bytes():
    from video_vae_amd import data as D
    clip = _clip((19, 23))
    got = D.resize_reference_u8(clip, 19, 23)
    assert got is not clip and np.array_equal(got, clip)


def test_exact_2x_is_the_four_tap_mean_rounded_half_to_even():
    """64 -> 32: src = 2 d + 0.5, both weights 0.5: the value is the mean of a 2 x 2 block, exact in fp32; a quarter of them end in .5."""
    from video_vae_amd import data as D
    clip = _clip((64, 64))
    s = clip.astype(np.int64)
    tot = s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]
    q, r = tot // 4, tot % 4
    want = np.where(r < 2, q, np.where(r > 2, q + 1, q + (q & 1)))
    assert 0.15 < float((r == 2).mean()) < 0.35                               # the ties are there
    assert np.array_equal(D.resize_reference_u8(clip, 32, 32), want.astype(np.uint8))


def test_reference_rejects_other_inputs():
    from video_vae_amd import data as D
    with pytest.raises(ValueError):
        D.resize_reference_u8(np.zeros((2, 4, 4, 3), dtype=np.float32), 2, 2)
    with pytest.raises(ValueError):
        D.resize_reference_u8(np.zeros((4, 4, 3), dtype=np.uint8), 2, 2)


def test_centre_square_crop_rule():
    from video_vae_amd import data as D
    assert D.centre_square_crop(45, 80) == (0, 17, 45) and D.centre_square_crop(20, 12) == (4, 0, 12) and D.centre_square_crop(7, 7) == (0, 0, 7)


def test_library_exports_the_resize_symbols_and_limits():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    l = lib()
    for name in ("vvae_crop_resize_supported", "vvae_crop_resize_u8"):
        assert name in protos and getattr(l, name) is not None
    assert len(protos["vvae_crop_resize_supported"][1]) == 7 and len(protos["vvae_crop_resize_u8"][1]) == 13
    ok = l.vvae_crop_resize_supported
    assert ok(720, 1280, 3, 720, 720, 256, 256) == 1 and ok(16384, 16384, 4, 1, 1, 1, 1) == 1 and ok(1, 1, 1, 1, 1, 16384, 16384) == 1
    for bad in ((16385, 8, 3, 8, 8, 4, 4), (8, 16385, 3, 8, 8, 4, 4), (8, 8, 0, 8, 8, 4, 4), (8, 8, 5, 8, 8, 4, 4), (8, 8, 3, 0, 8, 4, 4),
                (8, 8, 3, 8, 9, 4, 4), (8, 8, 3, 8, 8, 0, 4), (8, 8, 3, 8, 8, 4, 16385)):
        assert ok(*bad) == 0, bad


def test_crop_resize_needs_uint8_on_a_gpu():
    from video_vae_amd import ops
    with pytest.raises(ops.VvaeError):
        ops.crop_resize_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 0, 0, 8, 8, 4, 4)


def test_parser_takes_device_resize_and_refuses_it_with_tile():
    from video_vae_amd import infer
    base = ["--model_path", "m", "--data", "d"]
    for cmd, out in (("encode", ["--out", "o"]), ("eval", [])):
        assert infer.parse_args([cmd] + base + out).device_resize is False
        a = infer.parse_args([cmd] + base + out + ["--device-resize", "--scene-cuts", "--temporal-overlap", "2"])
        assert a.device_resize is True and a.tile is False
        with pytest.raises(SystemExit) as e:
            infer.parse_args([cmd] + base + out + ["--device-resize", "--tile"])
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        infer.parse_args(["scenes", "--data", "d", "--device-resize"])
    with pytest.raises(SystemExit):
        infer.parse_args(["decode", "--model_path", "m", "--latents", "l", "--out", "o", "--device-resize"])
