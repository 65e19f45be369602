"""Host: the training loader's plane mode for .y4m clips.  y4m.Y4MClip.window + y4m.window_to_rgb_reference equal the crop of
yuv_to_rgb_reference on the whole planes for every crop that fits a frame; the padding value is RGB zero; the ``device_yuv`` loader hands
over planes whose reference composition is the host loader's batch; the refusals; the ``train`` arguments; the ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FORMS = {"420_centre": ("420", "centre"), "420_mpeg2": ("420", "mpeg2"), "444": ("444", "centre"), "mono": ("mono", "centre")}
COLOURS = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]


def _planes(rng, t, h, w, chroma):
    from video_vae_amd import y4m
    y = rng.integers(0, 256, size=(t, h, w), dtype=np.uint8)
    if chroma == "mono":
        return y, None, None
    cs = (t,) + y4m.chroma_shape(h, w, chroma)
    return y, rng.integers(0, 256, size=cs, dtype=np.uint8), rng.integers(0, 256, size=cs, dtype=np.uint8)


def _tagged(path, planes, chroma, siting):
    """y4m.write, with the C tag rewritten for the mpeg2 siting (the writer tags 4:2:0 as C420jpeg)."""
    from video_vae_amd import y4m
    y4m.write(path, planes, chroma=chroma)
    if siting == "mpeg2":
        raw = open(path, "rb").read()
        assert raw.count(b" C420jpeg ") == 1
        open(path, "wb").write(raw.replace(b" C420jpeg ", b" C420mpeg2 ", 1))
    return path


@pytest.mark.parametrize("size", [(9, 11), (12, 10)], ids=["9x11", "12x10"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_window_equals_the_crop_of_the_whole_frame(tmp_path, form, size):
    """Every (top, left, h, w) that fits the frame: all four parities, odd and even sides, crops on every edge and corner, where the
    clamp acts.  The window is cut once per crop and converted with all four matrix / range pairs.  The largest chroma index a consumer
    reads is also checked against the window's shape: the + 3 is enough and is needed."""
    from video_vae_amd import y4m
    chroma, siting = FORMS[form]
    H, W = size
    planes = _planes(np.random.default_rng(H * 100 + W + len(form)), 2, H, W, chroma)
    clip = y4m.Y4MClip(_tagged(str(tmp_path / "a.y4m"), planes, chroma, siting))
    assert (clip.chroma, clip.siting) == (chroma, siting)
    whole = {c: y4m.yuv_to_rgb_reference(*planes, chroma, siting, *c) for c in COLOURS}
    cases, deepest = 0, 0
    for top in range(H):
        for h in range(1, H - top + 1):
            for left in range(W):
                for w in range(1, W - left + 1):
                    win = clip.window(0, 2, top, left, h, w)
                    assert win[0].shape == (2, h, w)
                    if chroma == "mono":
                        assert win[1] is None and win[2] is None
                    else:
                        assert win[1].shape == win[2].shape == (2,) + y4m.window_chroma_shape(h, w, chroma)
                    if chroma == "420":
                        assert win[1].shape == (2, h // 2 + 3, w // 2 + 3)
                        deepest = max(deepest, (((top & 1) + h - 1) >> 1) + 2 - (h // 2 + 2), (((left & 1) + w - 1) >> 1) + 2 - (w // 2 + 2))
                    for c in COLOURS:
                        got = y4m.window_to_rgb_reference(*win, (top & 1, left & 1), chroma, siting, *c)
                        assert np.array_equal(got, whole[c][:, top:top + h, left:left + w]), (top, left, h, w, c)
                    cases += 1
    assert cases == (H * (H + 1) // 2) * (W * (W + 1) // 2)
    assert deepest == 0                                                   # some crop reads the window's last row or column, none reads past it


@pytest.mark.parametrize("name", ["y4m_small.y4m", "y4m_small_444.y4m", "y4m_small_mono.y4m", "y4m_small_mpeg2.y4m"])
def test_windows_of_the_committed_clips(name):
    from video_vae_amd import y4m
    clip = y4m.Y4MClip(os.path.join(GOLDEN, name))
    t, H, W, _ = clip.shape
    whole = clip[0:t]
    rng = np.random.default_rng(3)
    crops = [(0, 0, H, W), (H - 1, W - 1, 1, 1), (0, W - 1, H, 1)]
    for _ in range(40):
        top, left = int(rng.integers(0, H)), int(rng.integers(0, W))
        crops.append((top, left, int(rng.integers(1, H - top + 1)), int(rng.integers(1, W - left + 1))))
    for top, left, h, w in crops:
        win = clip.window(0, t, top, left, h, w)
        got = y4m.window_to_rgb_reference(*win, (top & 1, left & 1), clip.chroma, clip.siting, clip.matrix, clip.full)
        assert np.array_equal(got, whole[:, top:top + h, left:left + w]), (name, top, left, h, w)
    for bad in ((0, 0, H + 1, W), (1, 0, H, W), (0, -1, 1, 1), (0, 0, 0, 1)):
        with pytest.raises(ValueError, match="does not lie inside"):
            clip.window(0, 1, *bad)
    with pytest.raises(ValueError, match="frames"):
        clip.window(0, t + 1, 0, 0, 1, 1)


def test_window_across_runs_of_different_frame_lines(tmp_path):
    from video_vae_amd import y4m
    H, W = 10, 14
    y, u, v = _planes(np.random.default_rng(8), 5, H, W, "420")
    path = str(tmp_path / "runs.y4m")
    with open(path, "wb") as fh:
        fh.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip C420jpeg\n".encode())
        for i, line in enumerate([b"FRAME\n", b"FRAME\n", b"FRAME Xfoo=1\n", b"FRAME Xfoo=1\n", b"FRAME\n"]):
            fh.write(line + y[i].tobytes() + u[i].tobytes() + v[i].tobytes())
    clip = y4m.Y4MClip(path)
    assert len(clip.runs()) == 3
    whole = y4m.yuv_to_rgb_reference(y, u, v)
    for a, b in ((0, 5), (1, 4), (2, 3), (3, 3)):
        win = clip.window(a, b, 3, 5, 6, 7)
        assert win[0].shape[0] == b - a
        assert np.array_equal(y4m.window_to_rgb_reference(*win, (1, 1)), whole[a:b, 3:9, 5:12])


def test_padding_value_is_rgb_zero():
    from video_vae_amd import y4m
    for matrix, full in COLOURS:
        for chroma, siting in FORMS.values():
            y = np.full((1, 5, 6), y4m.pad_luma(full), dtype=np.uint8)
            c = None if chroma == "mono" else np.full((1,) + y4m.window_chroma_shape(5, 6, chroma), y4m.PAD_CHROMA, dtype=np.uint8)
            for parity in ((0, 0), (0, 1), (1, 0), (1, 1)):
                assert not y4m.window_to_rgb_reference(y, c, c, parity, chroma, siting, matrix, full).any()


# ------------------------------------------------------------------------------------------------ the loader
FRAMES, CROP, SIZE = 6, 20, 16


def _folder(tmp_path, full=False):
    """Five 24 x 40 4:2:0 clips (clip0000 and clip0003 short) and one truncated file, which must come out as the zero fallback."""
    from video_vae_amd import data as D, y4m
    d = D.write_synthetic_clips(str(tmp_path), 5, FRAMES, 24, 40, seed=2, ext=".y4m")
    if full:
        for name in sorted(os.listdir(d)):
            clip = y4m.Y4MClip(os.path.join(d, name))
            planes = tuple(np.array(p) for p in clip.planes(0, len(clip)))      # copies: the file is rewritten under the memory map
            del clip
            y4m.write(os.path.join(d, name), planes, chroma="420", full=True)
    raw = open(os.path.join(d, "clip0001.y4m"), "rb").read()
    open(os.path.join(d, "cut0005.y4m"), "wb").write(raw[:len(raw) - 100])
    return str(tmp_path)


def _loader(base, **kw):
    from video_vae_amd import data as D
    a = dict(batch_size=2, max_frames=FRAMES, resize=(SIZE, SIZE), crop_size=CROP, shuffle=True, seed=3, num_workers=0, as_uint8=True)
    a.update(kw)
    return D.create_batched_dataloader(base, **a)


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("colour", ["bt601_header", "bt709_full"])
def test_plane_batches_compose_to_the_host_batches(tmp_path, capsys, workers, colour):
    from video_vae_amd import data as D, y4m
    matrix = colour.split("_")[0]
    full = colour.endswith("full")
    base = _folder(tmp_path, full=full)
    conf = None if colour == "bt601_header" else {"matrix": matrix, "range": "header"}
    host = list(_loader(base, num_workers=workers, y4m=conf))
    planes_loader = _loader(base, num_workers=workers, device_yuv=True, y4m=conf)
    assert planes_loader.yuv == {"chroma": "420", "siting": "centre", "matrix": matrix}
    planes = list(planes_loader)
    assert len(host) == len(planes) == 3
    short = fallback = 0
    for a, b in zip(host, planes):
        n = a["video"].shape[0]
        assert sorted(b) == ["mask", "params", "u", "v", "y"]
        assert b["y"].dtype == torch.uint8 and tuple(b["y"].shape) == (n, FRAMES, CROP, CROP)
        assert tuple(b["u"].shape) == tuple(b["v"].shape) == (n, FRAMES, CROP // 2 + 3, CROP // 2 + 3)
        assert b["params"].dtype == torch.int32 and tuple(b["params"].shape) == (n, 4)
        assert torch.equal(a["mask"], b["mask"])
        for i in range(n):
            py, px, rng_full, zero = (int(x) for x in b["params"][i])
            assert zero == 0 and py in (0, 1) and px in (0, 1)
            rgb = y4m.window_to_rgb_reference(b["y"][i].numpy(), b["u"][i].numpy(), b["v"][i].numpy(), (py, px), "420", "centre", matrix,
                                              bool(rng_full))
            want = D.resize_reference_u8(rgb, SIZE, SIZE)
            assert np.array_equal(want, a["video"][i].numpy())
            real = int(a["mask"][i].sum())
            if not a["video"][i].any():
                assert real == FRAMES                                     # the truncated file: zeros with an all-ones mask
                fallback += 1
            else:
                assert rng_full == int(full)
                short += real < FRAMES
                assert not a["video"][i, real:].any()                     # padding behind a short clip is RGB zero in both modes
    assert short == 2 and fallback == 1
    capsys.readouterr()


def test_host_path_takes_the_matrix_and_range(tmp_path):
    """y4m= reaches the host conversion too: another matrix or range gives other bytes; the default is what it was."""
    base = _folder(tmp_path)
    default = list(_loader(base))
    same = list(_loader(base, y4m={"matrix": "bt601", "range": "header"}))
    bt709 = list(_loader(base, y4m={"matrix": "bt709"}))
    full = list(_loader(base, y4m={"range": "full"}))
    assert all(torch.equal(a["video"], b["video"]) for a, b in zip(default, same))
    assert not all(torch.equal(a["video"], b["video"]) for a, b in zip(default, bt709))
    assert not all(torch.equal(a["video"], b["video"]) for a, b in zip(default, full))


def test_one_rng_picks_the_same_window_and_crop(tmp_path, capsys):
    from video_vae_amd import data as D, y4m
    base = _folder(tmp_path)
    for name in ("clip0000.y4m", "clip0001.y4m", "cut0005.y4m"):
        path = f"{base}/videos0/{name}"
        ra, rb = np.random.default_rng(9), np.random.default_rng(9)
        va, ma = D.load_video_u8(path, 4, (SIZE, SIZE), CROP, ra)
        y, u, v, params, mb = D.load_video_planes(path, 4, CROP, rb, None, ("420", "centre"))
        assert np.array_equal(ma, mb) and ra.integers(0, 1 << 30) == rb.integers(0, 1 << 30)
        assert y.shape == (4, CROP, CROP) and u.shape == v.shape == (4, CROP // 2 + 3, CROP // 2 + 3) and params.dtype == np.int32
        rgb = y4m.window_to_rgb_reference(y, u, v, params[:2], "420", "centre", "bt601", bool(params[2]))
        assert np.array_equal(D.resize_reference_u8(rgb, SIZE, SIZE), va)
    y, u, v, params, m = D.load_video_planes(f"{base}/videos0/clip0001.y4m", 4, CROP, np.random.default_rng(0), None, ("444", "centre"))
    assert (m == 1).all() and (y == 16).all() and (u == 128).all() and u.shape == (4, CROP, CROP)      # not the dataset's form
    capsys.readouterr()


def test_refusals_name_the_file(tmp_path):
    from video_vae_amd import data as D, y4m
    base = _folder(tmp_path / "ok")
    with pytest.raises(ValueError, match="as_uint8"):
        _loader(base, device_yuv=True, as_uint8=False)
    with pytest.raises(ValueError, match=r"clip0000\.y4m has frames of 24x40, below the crop 25"):
        _loader(base, device_yuv=True, crop_size=25)
    mixed = _folder(tmp_path / "npy")
    np.save(f"{mixed}/videos0/clip0002a.npy", np.zeros((2, 24, 40, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"clip0002a\.npy is not a \.y4m clip"):
        _loader(mixed, device_yuv=True)
    assert len(list(_loader(mixed))) == 4                                 # the host path still takes the mixed folder
    forms = _folder(tmp_path / "forms")
    y4m.write(f"{forms}/videos0/clip0003.y4m", np.zeros((2, 24, 40, 3), dtype=np.uint8), chroma="444")
    with pytest.raises(ValueError, match=r"clip0003\.y4m is 444 .* but .*clip0000\.y4m is 420"):
        _loader(forms, device_yuv=True)
    with pytest.raises(ValueError, match="resize"):
        D.DevicePrefetcher.__init__(object.__new__(D.DevicePrefetcher), [], "cpu", yuv={"chroma": "420", "siting": "centre", "matrix": "bt601"})


def test_train_arguments(monkeypatch, capsys):
    from video_vae_amd import data as D, train
    for bad in (["--device-yuv"], ["--data", "d", "--y4m-matrix", "bt2020"], ["--data", "d", "--y4m-range", "tv"]):
        with pytest.raises(SystemExit) as e:
            train.main(bad)                                               # an argument error: raised before a GPU is touched
        assert e.value.code == 2
    assert "--device-yuv needs --data" in capsys.readouterr().err
    seen = []

    class Host:
        yuv = {"chroma": "420", "siting": "mpeg2", "matrix": "bt709"}

    monkeypatch.setattr(D, "create_batched_dataloader", lambda directory, **kw: seen.append(kw) or Host())
    monkeypatch.setattr(D, "DevicePrefetcher", lambda host, dev, **kw: seen.append(kw) or "device")
    args = train.parse_args(["--data", "d", "--crop_size", "512", "--device-yuv", "--y4m-matrix", "bt709", "--y4m-range", "full"])
    assert args.device_yuv is True and args.device_resize is False
    assert train.data_batches(args, "d", 2, 8, 0, 0, "dev") == "device"
    assert seen[0]["device_yuv"] is True and seen[0]["y4m"] == {"matrix": "bt709", "range": "full"} and seen[0]["as_uint8"]
    assert seen[0]["crop_size"] == 512 and seen[0]["resize"] == (256, 256)
    assert seen[1]["yuv"] == Host.yuv and seen[1]["resize"] == (256, 256) and seen[1]["dtype"] == torch.bfloat16
    del seen[:]
    train.data_batches(train.parse_args(["--data", "d", "--y4m-matrix", "bt709"]), "d", 2, 8, 0, 0, "dev")
    assert "device_yuv" not in seen[0] and seen[0]["y4m"] == {"matrix": "bt709", "range": "header"}
    assert seen[1]["resize"] is None and "yuv" not in seen[1]
    del seen[:]
    args = train.parse_args(["--data", "d"])
    assert args.device_yuv is False and args.y4m_matrix == "bt601" and args.y4m_range == "header"
    train.data_batches(args, "d", 2, 8, 0, 0, "dev")
    assert "device_yuv" not in seen[0] and "y4m" not in seen[0] and "yuv" not in seen[1]      # without the flags: what was passed before


def test_abi_declares_and_exports_the_window_entries():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    ret, args = protos["vvae_yuv_window_supported"]
    assert ret is ctypes.c_int and args == [ctypes.c_int] * 5
    ret, args = protos["vvae_yuv_window_resize_norm"]
    assert ret is ctypes.c_int and len(args) == 16
    assert args[:5] == [ctypes.c_void_p] * 5 and args[-1] is ctypes.c_void_p and all(a is ctypes.c_int for a in args[5:-1])
    assert callable(lib().vvae_yuv_window_supported) and callable(lib().vvae_yuv_window_resize_norm)
    assert len(protos["vvae_yuv_to_rgb_u8"][1]) == 14 and len(protos["vvae_crop_resize_norm"][1]) == 14      # the neighbours keep theirs
    f = lib().vvae_yuv_window_supported
    assert f(1, 1, 0, 1, 1) and f(16384, 16384, 2, 16384, 16384)
    assert not f(0, 4, 0, 4, 4) and not f(4, 16385, 0, 4, 4) and not f(4, 4, 3, 4, 4) and not f(4, 4, -1, 4, 4) and not f(4, 4, 0, 4, 0)
    assert not f(4, 4, 0, 16385, 4)
    # a refused call returns before anything touches a device
    assert lib().vvae_yuv_window_resize_norm(None, None, None, None, None, 0, 1, 1, 4, 4, 2, 0, 0, 4, 4, None) == 1001
    assert protos["vvae_yuv_window_span"] == (ctypes.c_int, []) and lib().vvae_yuv_window_span() >= 64
