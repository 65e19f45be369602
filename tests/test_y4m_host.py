"""CPU: the YUV4MPEG2 module (video_vae_amd/y4m.py) -- header parsing and its refusals, the colour arithmetic against the fixture's
independent scalar loop, greys and round trips within the derived bounds, the writer, the loader's .y4m branch and infer's options."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"420": "y4m_small.y4m", "420mpeg2": "y4m_small_mpeg2.y4m", "444": "y4m_small_444.y4m", "mono": "y4m_small_mono.y4m"}
FORMS = {"420": ("420", "centre"), "420mpeg2": ("420", "mpeg2"), "444": ("444", "centre"), "mono": ("mono", "centre")}


def _file(tmp_path, head, frames=1, frame=b"FRAME\n", payload=None, name="clip.y4m"):
    p = tmp_path / name
    p.write_bytes(head + b"".join(frame + payload for _ in range(frames)) if payload is not None else head)
    return str(p)


def test_header_parsing_and_tag_order():
    from video_vae_amd import y4m
    h = y4m.read_header(os.path.join(GOLDEN, FILES["420"]))
    assert (h.width, h.height, h.fps, h.interlace, h.aspect, h.chroma, h.siting, h.full) == (7, 5, (30000, 1001), "p", (1, 1), "420",
                                                                                            "centre", None)
    assert h.extra == ["XYSCSS=420JPEG"] and h.chroma_shape == (3, 4) and h.frame_bytes == 35 + 24
    h = y4m.read_header(os.path.join(GOLDEN, FILES["420mpeg2"]))                       # H before W, C before F, no I tag
    assert (h.width, h.height, h.fps, h.chroma, h.siting, h.interlace) == (7, 5, (25, 1), "420", "mpeg2", "?")
    h = y4m.read_header(os.path.join(GOLDEN, FILES["444"]))
    assert (h.chroma, h.full, h.chroma_shape) == ("444", True, (5, 7))
    h = y4m.read_header(os.path.join(GOLDEN, FILES["mono"]))
    assert (h.chroma, h.interlace, h.frame_bytes) == ("mono", "?", 35)
    assert y4m.parse_header(b"YUV4MPEG2 W4 H2").chroma == "420" and y4m.parse_header(b"YUV4MPEG2 W4 H2 C420\n").siting == "centre"
    assert y4m.parse_header(b"YUV4MPEG2 W4 H2 XCOLORRANGE=LIMITED\n").full is False


@pytest.mark.parametrize("tag", ["C420paldv", "C422", "C411", "C444alpha", "C420p10", "C422p10", "C444p12", "C420p16", "Cmono16",
                                 "It", "Ib", "Im"])
def test_refused_tags_name_the_file_and_the_tag(tmp_path, tag):
    from video_vae_amd import y4m
    path = _file(tmp_path, f"YUV4MPEG2 W4 H2 F30:1 {tag}\n".encode(), payload=bytes(12))
    for fn in (y4m.read_header, y4m.Y4MClip):
        with pytest.raises(ValueError) as e:
            fn(path)
        assert tag in str(e.value) and path in str(e.value)


def test_refused_sizes_and_frames(tmp_path):
    from video_vae_amd import y4m
    cases = {"W": b"YUV4MPEG2 H2 F30:1\n", "H": b"YUV4MPEG2 W4 F30:1\n", "W16385": b"YUV4MPEG2 W16385 H2\n", "H20000": b"YUV4MPEG2 W4 H20000\n"}
    for what, head in cases.items():
        path = _file(tmp_path, head)
        with pytest.raises(ValueError) as e:
            y4m.read_header(path)
        assert what in str(e.value) and path in str(e.value)
    assert y4m.parse_header(b"YUV4MPEG2 W16384 H16384\n").width == 16384
    head = b"YUV4MPEG2 W4 H2 C420jpeg\n"
    ok = _file(tmp_path, head, frames=2, payload=bytes(12))
    assert y4m.Y4MClip(ok).shape == (2, 2, 4, 3)
    assert y4m.Y4MClip(_file(tmp_path, head, name="empty.y4m")).shape == (0, 2, 4, 3)
    bad = tmp_path / "noframe.y4m"
    bad.write_bytes(head + b"FRAME\n" + bytes(12) + b"FRAMX\n" + bytes(12))
    with pytest.raises(ValueError, match="FRAME") as e:
        y4m.Y4MClip(str(bad))
    assert str(bad) in str(e.value)
    raw = tmp_path / "raw.y4m"
    raw.write_bytes(head + bytes(12))                                                  # planes without a FRAME line
    with pytest.raises(ValueError, match="FRAME"):
        y4m.Y4MClip(str(raw))
    short = tmp_path / "short.y4m"
    short.write_bytes(head + b"FRAME\n" + bytes(12) + b"FRAME\n" + bytes(11))
    with pytest.raises(ValueError, match="cut short") as e:
        y4m.Y4MClip(str(short))
    assert str(short) in str(e.value)
    notmagic = _file(tmp_path, b"YUV4MPEG3 W4 H2\n", name="magic.y4m")
    with pytest.raises(ValueError):
        y4m.read_header(notmagic)


@pytest.mark.parametrize("form", sorted(FILES))
def test_reference_equals_the_fixture_s_scalar_loop(form):
    from video_vae_amd import y4m
    with np.load(os.path.join(GOLDEN, "y4m_small_rgb.npz")) as z:
        want = {k: z[k] for k in z.files}
    path = os.path.join(GOLDEN, FILES[form])
    for matrix in ("bt601", "bt709"):
        for rng in ("limited", "full"):
            clip = y4m.Y4MClip(path, matrix=matrix, range=rng)
            assert clip.shape == (3, 5, 7, 3) and (clip.chroma, clip.siting) == FORMS[form]
            got = clip[0:3]
            assert got.dtype == np.uint8 and np.array_equal(got, want[f"{form}_{matrix}_{rng}"]), (form, matrix, rng)
            assert np.array_equal(clip[1:2], got[1:2]) and np.array_equal(clip[2], got[2]) and np.array_equal(clip[-1], got[2])
            assert clip[3:7].shape == (0, 5, 7, 3)
    hdr = y4m.Y4MClip(path)                                                            # range="header": full only where the file says so
    assert hdr.full == (form == "444")
    assert np.array_equal(hdr[:], want[f"{form}_bt601_{'full' if form == '444' else 'limited'}"])


def test_frame_lines_of_different_lengths_are_walked():
    from video_vae_amd import y4m
    clip = y4m.Y4MClip(os.path.join(GOLDEN, FILES["420"]))
    assert clip.lines.tolist() == [6, 9, 6] and clip.runs() == [(0, 1), (1, 2), (2, 3)]
    assert clip.starts.tolist() == [clip.header.size, clip.header.size + 65, clip.header.size + 65 + 68]
    with pytest.raises(ValueError):
        clip.planes(0, 2)
    same = y4m.Y4MClip(os.path.join(GOLDEN, FILES["444"]))
    assert same.runs() == [(0, 3)] and same.runs(0, 3, run_bytes=1) == [(0, 1), (1, 2), (2, 3)]
    assert same.runs(1, 3, run_bytes=2 * (105 + 80)) == [(1, 3)]


def test_greys_and_white():
    from video_vae_amd import y4m
    g = np.arange(256, dtype=np.uint8)
    rgb = np.stack([g, g, g], axis=-1).reshape(1, 16, 16, 3)
    for matrix in y4m.MATRICES:
        for full in (False, True):
            for chroma in ("420", "444"):
                y, u, v = y4m.rgb_to_yuv_reference(rgb, chroma, matrix, full)
                assert (u == 128).all() and (v == 128).all(), (matrix, full, chroma)
                assert int(y.reshape(-1)[255]) == (255 if full else 235) and int(y.reshape(-1)[0]) == (0 if full else 16)
            # constant grey frames: R = G = B back, within 1 (limited) and exactly (full)
            flat = np.broadcast_to(g[:, None, None, None], (256, 2, 2, 3)).copy()
            back = y4m.yuv_to_rgb_reference(*y4m.rgb_to_yuv_reference(flat, "420", matrix, full), "420", "centre", matrix, full).astype(int)
            assert (back[..., 0] == back[..., 1]).all() and (back[..., 1] == back[..., 2]).all()
            assert np.abs(back - flat).max() <= (0 if full else 1), (matrix, full)


def test_constant_colour_round_trip_within_the_derived_bounds():
    from video_vae_amd import y4m
    rng = np.random.default_rng(5)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8)
    colours = np.concatenate([corners, rng.integers(0, 256, size=(4088, 3), dtype=np.uint8)])
    flat = np.broadcast_to(colours[:, None, None, :], (4096, 3, 3, 3)).copy()          # 3 x 3: odd edges, replicated blocks
    for matrix in y4m.MATRICES:
        for full in (False, True):
            for chroma, siting in (("420", "centre"), ("420", "mpeg2"), ("444", "centre")):
                y, u, v = y4m.rgb_to_yuv_reference(flat, chroma, matrix, full)
                back = y4m.yuv_to_rgb_reference(y, u, v, chroma, siting, matrix, full).astype(int)
                err = int(np.abs(back - flat).max())
                print(matrix, full, chroma, siting, err)
                assert err <= (1 if full else 2), (matrix, full, chroma, siting, err)


def test_write_then_planes_returns_the_written_planes(tmp_path):
    from video_vae_amd import y4m
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, size=(4, 9, 13, 3), dtype=np.uint8)
    for chroma in ("420", "444"):
        for full in (False, True):
            path = str(tmp_path / f"w_{chroma}_{full}.y4m")
            y4m.write(path, rgb, fps=(25, 2), chroma=chroma, matrix="bt709", full=full)
            h = y4m.read_header(path)
            assert (h.width, h.height, h.fps, h.interlace, h.chroma, h.siting, h.full) == (13, 9, (25, 2), "p", chroma, "centre", full)
            assert h.tag == ("420jpeg" if chroma == "420" else "444")
            clip = y4m.Y4MClip(path, matrix="bt709")
            assert clip.full == full and clip.shape == (4, 9, 13, 3)
            want = y4m.rgb_to_yuv_reference(rgb, chroma, "bt709", full)
            got = clip.planes(0, 4)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)
                assert not a.flags.owndata and not a.flags.writeable                   # views of the memory map
            assert np.array_equal(clip.planes(1, 3)[1], want[1][1:3])
            again = str(tmp_path / "again.y4m")
            y4m.write(again, want, fps="25:2", chroma=chroma, full=full)               # planes are written as they are
            assert open(again, "rb").read() == open(path, "rb").read()
    mono = str(tmp_path / "mono.y4m")
    y4m.write(mono, (rgb[..., 0], None, None), chroma="mono")
    m = y4m.Y4MClip(mono)
    assert m.chroma == "mono" and np.array_equal(m.planes(0, 4)[0], rgb[..., 0]) and m.planes(0, 4)[1] is None
    assert (m[0][..., 0] == m[0][..., 1]).all()


def test_loader_reads_y4m_like_the_npy_of_its_rgb(tmp_path, capsys):
    from video_vae_amd import data as D
    from video_vae_amd import y4m
    rng = np.random.default_rng(7)
    d = tmp_path / "videos0"
    d.mkdir()
    y4m.write(str(d / "a.y4m"), rng.integers(0, 256, size=(9, 40, 52, 3), dtype=np.uint8))
    ref = y4m.Y4MClip(str(d / "a.y4m"))[:]
    np.save(d / "b.npy", ref)
    assert D.list_video_files(str(tmp_path)) == [str(d / "a.y4m"), str(d / "b.npy")]
    for kw in (dict(max_frames=4, resize=(16, 16), crop_size=32), dict(max_frames=12, resize=None, crop_size=48),
               dict(max_frames=4, resize=(16, 16), crop_size=32, device_resize=True)):
        a = D.load_video_u8(str(d / "a.y4m"), rng=np.random.default_rng(3), **kw)
        b = D.load_video_u8(str(d / "b.npy"), rng=np.random.default_rng(3), **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()
    frames, total = D._read_frames(str(d / "a.y4m"), lambda t: t - 2, 5)               # a callable start, as for arrays
    assert total == 9 and np.array_equal(frames, ref[7:9])
    frames, _ = D._read_frames(str(d / "a.y4m"), 2, 3, {"matrix": "bt709", "range": "full"})
    assert np.array_equal(frames, y4m.Y4MClip(str(d / "a.y4m"), "bt709", "full")[2:5]) and not np.array_equal(frames, ref[2:5])
    whole = open(d / "a.y4m", "rb").read()
    (d / "cut.y4m").write_bytes(whole[:-100])
    v, m = D.load_video_u8(str(d / "cut.y4m"), 4, (16, 16), 32, np.random.default_rng(3))
    assert v.shape == (4, 16, 16, 3) and not v.any() and (m == 1).all()                 # the zero-clip fallback
    assert "cut short" in capsys.readouterr().out


def test_batch_to_video_y4m_reads_back(tmp_path):
    from video_vae_amd import data as D
    from video_vae_amd import y4m
    g = torch.Generator().manual_seed(8)
    video = torch.rand((1, 5, 10, 14, 3), generator=g) * 1.2 - 0.1
    mask = torch.tensor([[1.0, 1.0, 1.0, 0.0, 0.0]])
    path = str(tmp_path / "out.y4m")
    D.batch_to_video({"video": video, "mask": mask}, path, fps=(24, 1), y4m={"chroma": "444", "matrix": "bt709", "full": True})
    u8 = (np.clip(video[0, :3].numpy(), 0, 1) * 255).astype(np.uint8)
    clip = y4m.Y4MClip(path, matrix="bt709")
    assert clip.header.fps == (24, 1) and clip.chroma == "444" and clip.full and clip.shape == (3, 10, 14, 3)
    for a, b in zip(clip.planes(0, 3), y4m.rgb_to_yuv_reference(u8, "444", "bt709", True)):
        assert np.array_equal(a, b)
    assert np.abs(clip[:].astype(int) - u8).max() <= 1                                 # 4:4:4 full range: one pixel's round trip
    D.batch_to_video({"video": video, "mask": mask}, str(tmp_path / "d.y4m"))
    d = y4m.Y4MClip(str(tmp_path / "d.y4m"))
    assert d.header.fps == (30, 1) and d.chroma == "420" and not d.full and d.header.tag == "420jpeg"


def test_parser_takes_the_y4m_options(tmp_path):
    from video_vae_amd import infer
    for cmd in ("encode", "eval", "scenes"):
        base = [cmd, "--data", "d", "--out", "o"] + ([] if cmd == "scenes" else ["--model_path", "m"])
        a = infer.parse_args(base)
        assert (a.y4m_matrix, a.y4m_range) == ("bt601", "header")
        a = infer.parse_args(base + ["--y4m-matrix", "bt709", "--y4m-range", "full"])
        assert (a.y4m_matrix, a.y4m_range) == ("bt709", "full") and infer._y4m_read(a) == {"matrix": "bt709", "range": "full"}
        for bad in (["--y4m-matrix", "foo"], ["--y4m-range", "video"]):
            with pytest.raises(SystemExit):
                infer.parse_args(base + bad)
    dec = ["decode", "--model_path", "m", "--latents", "l", "--out", "o"]
    a = infer.parse_args(dec)
    assert (a.ext, a.y4m_matrix, a.y4m_range, a.y4m_chroma, a.fps) == ("npz", "bt601", "limited", "420", "30:1")
    a = infer.parse_args(dec + ["--ext", "y4m", "--y4m-matrix", "bt709", "--y4m-range", "full", "--y4m-chroma", "444", "--fps", "30000:1001"])
    assert (a.ext, a.y4m_matrix, a.y4m_range, a.y4m_chroma, a.fps) == ("y4m", "bt709", "full", "444", "30000:1001")
    for bad in (["--ext", "foo"], ["--y4m-matrix", "foo"], ["--y4m-range", "header"], ["--y4m-chroma", "422"], ["--fps", "30"], ["--fps", "0:1"]):
        with pytest.raises(SystemExit):
            infer.parse_args(dec + bad)
    with pytest.raises(SystemExit, match=r"\.y4m"):                                    # the "no clips" message names the format
        infer._clip_paths(str(tmp_path))
