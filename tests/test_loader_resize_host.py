"""Host: the training loader's device-resize split (data.load_video_u8 / create_batched_dataloader with ``device_resize=True``) hands over
the crops whose resize_reference_u8 is the default loader's batch, byte for byte; the unreadable-clip fallback; the refusals; the ABI of
vvae_crop_resize_norm; the ``train`` arguments --crop_size and --device-resize."""
import numpy as np
import pytest
import torch

CROP, SIZE, FRAMES = 36, 32, 8


def _clips(tmp_path):
    """Six 40 x 48 clips (every third one short) and one 20 x 28 clip: smaller than the crop, so it takes the host upscale first."""
    from video_vae_amd import data as D
    d = D.write_synthetic_clips(str(tmp_path), 6, FRAMES, 40, 48)
    np.save(f"{d}/small0006.npy", np.random.default_rng(5).integers(0, 256, size=(FRAMES, 20, 28, 3), dtype=np.uint8))
    return str(tmp_path)


def _batches(base, **kw):
    from video_vae_amd import data as D
    return list(D.create_batched_dataloader(base, batch_size=2, max_frames=FRAMES, resize=(SIZE, SIZE), crop_size=CROP, shuffle=True, seed=3,
                                            num_workers=0, as_uint8=True, **kw))


def test_split_is_exact(tmp_path):
    from video_vae_amd import data as D
    base = _clips(tmp_path)
    host, split = _batches(base), _batches(base, device_resize=True)
    assert len(host) == len(split) == 4                                   # 7 clips in batches of 2, the last one single
    short = 0
    for a, b in zip(host, split):
        n = a["video"].shape[0]
        assert b["video"].dtype == torch.uint8 and tuple(b["video"].shape) == (n, FRAMES, CROP, CROP, 3)
        assert tuple(a["video"].shape) == (n, FRAMES, SIZE, SIZE, 3)
        assert torch.equal(a["mask"], b["mask"])
        short += int((a["mask"].sum(1) < FRAMES).sum())
        want = D.resize_reference_u8(b["video"].numpy().reshape(-1, CROP, CROP, 3), SIZE, SIZE).reshape(a["video"].shape)
        assert np.array_equal(want, a["video"].numpy())
    assert short == 2                                                     # the padded clips went through both modes


def test_one_rng_picks_the_same_window_and_crop_in_both_modes(tmp_path):
    """load_video_u8 itself, on the undersized clip and a full-size one: the rng ends in the same state whichever mode ran."""
    from video_vae_amd import data as D
    base = _clips(tmp_path)
    for name in ("small0006.npy", "clip0001.npy"):
        path = f"{base}/videos0/{name}"
        ra, rb = np.random.default_rng(9), np.random.default_rng(9)
        va, ma = D.load_video_u8(path, 5, (SIZE, SIZE), CROP, ra)
        vb, mb = D.load_video_u8(path, 5, (SIZE, SIZE), CROP, rb, device_resize=True)
        assert vb.shape == (5, CROP, CROP, 3) and np.array_equal(ma, mb) and ra.integers(0, 1 << 30) == rb.integers(0, 1 << 30)
        assert np.array_equal(D.resize_reference_u8(vb, SIZE, SIZE), va)


def test_unreadable_clip_is_zeros_at_crop_size(tmp_path, capsys):
    from video_vae_amd import data as D
    bad = tmp_path / "bad.npy"
    np.save(bad, np.zeros((4, 8, 8), dtype=np.float32))                   # not uint8 (T, H, W, 3)
    v, m = D.load_video_u8(str(bad), FRAMES, (SIZE, SIZE), CROP, np.random.default_rng(0), device_resize=True)
    assert v.dtype == np.uint8 and v.shape == (FRAMES, CROP, CROP, 3) and not v.any()
    assert m.dtype == np.float32 and m.shape == (FRAMES,) and (m == 1).all()
    v, m = D.load_video_u8(str(bad), FRAMES, (SIZE, SIZE), CROP, np.random.default_rng(0))
    assert v.shape == (FRAMES, SIZE, SIZE, 3) and (m == 1).all()          # the default mode's fallback is where it was
    capsys.readouterr()


def test_refusals(tmp_path):
    from video_vae_amd import data as D, ops
    base = _clips(tmp_path)
    with pytest.raises(ValueError, match="as_uint8"):
        D.create_batched_dataloader(base, batch_size=2, max_frames=FRAMES, resize=(SIZE, SIZE), crop_size=CROP, num_workers=0,
                                    as_uint8=False, device_resize=True)
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ops.VvaeError, match="on a GPU"):
        ops.crop_resize_norm(x, 0, 0, 8, 8, 4, 4)
    with pytest.raises(ops.VvaeError, match="float32 or bfloat16"):
        ops.crop_resize_norm(x, 0, 0, 8, 8, 4, 4, dtype=torch.float16)


def test_abi_declares_and_exports_crop_resize_norm():
    import ctypes
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    ret, args = protos["vvae_crop_resize_norm"]
    assert ret is ctypes.c_int and len(args) == 14
    assert args[:3] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] and args[-1] is ctypes.c_void_p
    assert all(a is ctypes.c_int for a in args[2:-1])
    assert callable(lib().vvae_crop_resize_norm)
    assert len(protos["vvae_crop_resize_u8"][1]) == 13                    # the byte entry keeps its signature


def test_train_arguments(monkeypatch, capsys):
    from video_vae_amd import data as D, train
    for bad in (["--size", "64", "--crop_size", "48", "--data", "d"], ["--device-resize"], ["--device-resize", "--crop_size", "512"]):
        with pytest.raises(SystemExit) as e:
            train.main(bad)                                               # an argument error: raised before a GPU is touched
        assert e.value.code == 2
    assert "--crop_size 48 is below --size 64" in capsys.readouterr().err
    seen = []
    monkeypatch.setattr(D, "create_batched_dataloader", lambda directory, **kw: seen.append(kw) or "host")
    monkeypatch.setattr(D, "DevicePrefetcher", lambda host, dev, **kw: seen.append(kw) or "device")
    args = train.parse_args(["--data", "d", "--size", "64"])
    assert args.crop_size == 64 and args.device_resize is False
    assert train.data_batches(args, "d", 2, 8, 0, 0, "dev") == "device"
    assert seen[0]["crop_size"] == 64 and seen[0]["resize"] == (64, 64) and seen[0]["device_resize"] is False and seen[0]["as_uint8"]
    assert seen[1]["resize"] is None
    del seen[:]
    args = train.parse_args(["--data", "d", "--crop_size", "512", "--device-resize"])
    train.data_batches(args, "e", 2, 8, 0, 0, "dev")
    assert seen[0]["crop_size"] == 512 and seen[0]["resize"] == (256, 256) and seen[0]["device_resize"] is True
    assert seen[1]["resize"] == (256, 256) and seen[1]["dtype"] == torch.bfloat16
    del seen[:]
    train.data_batches(train.parse_args(["--data", "d", "--crop_size", "512"]), "d", 2, 8, 0, 0, "dev")
    assert seen[0]["crop_size"] == 512 and seen[0]["device_resize"] is False and seen[1]["resize"] is None
