"""GPU: the colour-conversion kernels (csrc/yuv.hip) against their written specification (y4m.yuv_to_rgb_reference /
rgb_to_yuv_reference), byte for byte, zero tolerance: every geometry at which a thread, a workgroup or the grid takes another path, every
form x siting x matrix x range, planes taken as views of an uploaded record buffer at every alignment, poisoned margins, a captured launch,
the refusals; the run-by-run upload of a Y4MClip; ``infer encode|scenes|decode`` on .y4m clips against the same commands on the .npy of
their reference RGB."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = 0xA5
MARGIN = 64
# a thread owns 8 pixels of a row pair in both kernels (from RGB: 4 blocks), so a workgroup of 256 threads spans 2048 pixels of a row:
# 2050 is just past one workgroup, with a short last thread; 1026 is past half of one, with a last chroma dword cut by the row's end
GEOMETRIES = [(1, 1), (2, 2), (3, 5), (16, 16), (17, 31), (3, 1026), (3, 2050)]
GRID_CAP = 65535                                                   # YUV_MAX_GRID_Z: more frames than this are strided over
FORMS = [("420", "centre"), ("420", "mpeg2"), ("444", "centre"), ("mono", "centre")]


def _chroma_shape(h, w, chroma):
    return {"420": ((h + 1) // 2, (w + 1) // 2), "444": (h, w), "mono": (0, 0)}[chroma]


@functools.lru_cache(maxsize=None)
def _records(n, h, w, chroma, line, lead, seed=0):
    """A poisoned host buffer holding ``n`` frame records as a .y4m file lays them out (a FRAME line of ``line`` bytes, then the planes,
    uniform random bytes) behind MARGIN + lead bytes of poison and before MARGIN more -> (buffer, line offset of record 0, record stride).
    Computed once per case, shared and left unchanged."""
    ch, cw = _chroma_shape(h, w, chroma)
    stride = line + h * w + 2 * ch * cw
    rng = np.random.default_rng([seed, n, h, w, line, lead])
    buf = np.full(MARGIN + lead + n * stride + MARGIN, POISON, dtype=np.uint8)
    body = buf[MARGIN + lead:MARGIN + lead + n * stride].reshape(n, stride)
    body[:, :line] = np.frombuffer((b"FRAME" + b" Ip"[:line - 6] + b"\n").ljust(line, b"\n")[:line], dtype=np.uint8)
    body[:, line:] = rng.integers(0, 256, size=(n, stride - line), dtype=np.uint8)
    buf.setflags(write=False)
    return buf, MARGIN + lead, stride


def _views(buf, start, stride, n, h, w, chroma, line, strided):
    """(y, u, v) views of the records in ``buf`` (numpy array or torch tensor); ``strided(buf, shape, strides, offset)`` makes one."""
    ch, cw = _chroma_shape(h, w, chroma)
    y = strided(buf, (n, h, w), (stride, w, 1), start + line)
    if chroma == "mono":
        return y, None, None
    return (y, strided(buf, (n, ch, cw), (stride, cw, 1), start + line + h * w),
            strided(buf, (n, ch, cw), (stride, cw, 1), start + line + h * w + ch * cw))


def _np_strided(buf, shape, strides, offset):
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=shape, strides=strides, writeable=False)


def _torch_strided(buf, shape, strides, offset):
    return buf.as_strided(shape, strides, offset)


def _to_rgb_case(dev, n, h, w, chroma, siting, matrix, full, line, lead, out_offset=0):
    """Run ops.yuv_to_rgb_u8 on views of an uploaded record buffer into a view of a poisoned output buffer; hold the result against the
    reference and every byte outside it, the record buffer included, against what it was."""
    from video_vae_amd import ops, y4m
    host, start, stride = _records(n, h, w, chroma, line, lead)
    want = y4m.yuv_to_rgb_reference(*_views(host, start, stride, n, h, w, chroma, line, _np_strided), chroma, siting, matrix, full)
    buf = torch.from_numpy(np.array(host)).to(dev)
    y, u, v = _views(buf, start, stride, n, h, w, chroma, line, _torch_strided)
    size = n * h * w * 3
    obuf = torch.full((size + 2 * MARGIN,), POISON, dtype=torch.uint8, device=dev)
    out = obuf[MARGIN + out_offset:MARGIN + out_offset + size].view(n, h, w, 3)
    res = ops.yuv_to_rgb_u8(y, u, v, chroma, siting, matrix, full, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    got = obuf.cpu().numpy()
    lo, hi = MARGIN + out_offset, MARGIN + out_offset + size
    bad = int((got[lo:hi].reshape(want.shape) != want).sum())
    print(f"yuv_to_rgb n={n} {h}x{w} {chroma}/{siting} {matrix} full={full} line={line} lead={lead}: {bad} of {want.size} bytes differ; "
          f"plane bases mod 4: y {(start + line) % 4}" + ("" if u is None else f" u {u.storage_offset() % 4} v {v.storage_offset() % 4}"))
    assert bad == 0
    assert (got[:lo] == POISON).all() and (got[hi:] == POISON).all()
    assert np.array_equal(buf.cpu().numpy(), host)                                     # the source and its margins: untouched
    return want


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_yuv_to_rgb_equals_reference_at_every_geometry(dev, hw, n):
    for line in (6, 9):
        _to_rgb_case(dev, n, hw[0], hw[1], "420", "centre", "bt601", False, line, 0)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{f[0]}-{f[1]}")
def test_yuv_to_rgb_every_form_matrix_and_range(dev, form):
    for matrix in ("bt601", "bt709"):
        for full in (False, True):
            _to_rgb_case(dev, 3, 17, 31, form[0], form[1], matrix, full, 9, 0)
            _to_rgb_case(dev, 2, 3, 2050, form[0], form[1], matrix, full, 6, 0)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_yuv_to_rgb_plane_bases_at_every_residue(dev, lead):
    """FRAME lines of 6 and 9 bytes behind 0 .. 3 more bytes: every plane base, every record stride and the output fall on every residue
    mod 4; 16 x 16 and 4 x 8 have dword-sized rows, so the dword paths run where the base allows and the byte paths where it does not."""
    for line in (6, 9):
        for h, w, chroma in ((17, 31, "420"), (16, 16, "420"), (4, 8, "444"), (3, 5, "mono")):
            _to_rgb_case(dev, 3, h, w, chroma, "mpeg2" if chroma == "420" and lead % 2 else "centre", "bt709", bool(lead & 2), line, lead,
                         out_offset=lead)


def _from_rgb_case(dev, n, h, w, chroma, matrix, full, offset=0):
    from video_vae_amd import ops, y4m
    rng = np.random.default_rng([1, n, h, w])
    rgb = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    want = y4m.rgb_to_yuv_reference(rgb, chroma, matrix, full)
    bufs, outs = [], []
    for k, p in enumerate(want):
        b = torch.full((p.size + 2 * MARGIN,), POISON, dtype=torch.uint8, device=dev)
        bufs.append(b)
        o = MARGIN + (offset + k) % 4
        outs.append(b[o:o + p.size].view(p.shape))
    src = torch.full((rgb.size + 2 * MARGIN,), POISON, dtype=torch.uint8, device=dev)
    x = src[MARGIN + offset:MARGIN + offset + rgb.size].view(rgb.shape)
    x.copy_(torch.from_numpy(rgb))
    res = ops.rgb_to_yuv(x, chroma, matrix, full, out=tuple(outs))
    torch.cuda.synchronize()
    for k, (name, p) in enumerate(zip("yuv", want)):
        assert res[k].data_ptr() == outs[k].data_ptr()
        got = bufs[k].cpu().numpy()
        o = MARGIN + (offset + k) % 4
        bad = int((got[o:o + p.size].reshape(p.shape) != p).sum())
        print(f"rgb_to_yuv n={n} {h}x{w} {chroma} {matrix} full={full} offset={offset}: plane {name}: {bad} of {p.size} bytes differ")
        assert bad == 0
        assert (got[:o] == POISON).all() and (got[o + p.size:] == POISON).all()
    s = src.cpu().numpy()
    assert (s[:MARGIN + offset] == POISON).all() and (s[MARGIN + offset + rgb.size:] == POISON).all()
    free = ops.rgb_to_yuv(x, chroma, matrix, full)                                     # its own outputs
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(free, want))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_rgb_to_yuv_equals_reference_at_every_geometry(dev, hw, n):
    for offset in (0, 1):
        _from_rgb_case(dev, n, hw[0], hw[1], "420", "bt601", False, offset)


@pytest.mark.parametrize("chroma", ["420", "444"])
def test_rgb_to_yuv_every_form_matrix_and_range(dev, chroma):
    for matrix in ("bt601", "bt709"):
        for full in (False, True):
            for offset in (0, 2, 3):
                _from_rgb_case(dev, 3, 17, 31, chroma, matrix, full, offset)
            _from_rgb_case(dev, 2, 3, 2050, chroma, matrix, full)
            _from_rgb_case(dev, 2, 16, 16, chroma, matrix, full)


def test_more_frames_than_the_grid_s_frame_dimension(dev):
    """n just past the launcher's cap on gridDim.z at 2 x 2: the kernels stride over the frames."""
    n = GRID_CAP + 2
    _to_rgb_case(dev, n, 2, 2, "420", "centre", "bt601", False, 6, 0)
    _from_rgb_case(dev, n, 2, 2, "420", "bt601", False)


def test_captured_launches_replay_on_new_bytes(dev):
    from video_vae_amd import ops, y4m
    from video_vae_amd.graph import graph_node_census
    n, h, w, line = 3, 17, 31, 9
    host, start, stride = _records(n, h, w, "420", line, 0)
    buf = torch.from_numpy(np.array(host)).to(dev)
    y, u, v = _views(buf, start, stride, n, h, w, "420", line, _torch_strided)
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    planes = tuple(torch.empty(s, dtype=torch.uint8, device=dev) for s in ((n, h, w), (n, 9, 16), (n, 9, 16)))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def run():
        ops.yuv_to_rgb_u8(y, u, v, "420", "mpeg2", "bt709", False, out=rgb)
        ops.rgb_to_yuv(rgb, "420", "bt709", False, out=planes)

    with torch.cuda.stream(s):
        run()
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    census = graph_node_census(graph)
    assert census is None or census.get("memset", 0) == 0, census
    assert census is None or census.get("kernel", 2) == 2, census
    g = torch.Generator().manual_seed(12)
    for _ in range(2):
        new = torch.randint(0, 256, (buf.numel(),), generator=g, dtype=torch.uint8)
        buf.copy_(new)
        rgb.fill_(0)
        for p in planes:
            p.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        want = y4m.yuv_to_rgb_reference(*_views(new.numpy(), start, stride, n, h, w, "420", line, _np_strided), "420", "mpeg2", "bt709", False)
        assert np.array_equal(rgb.cpu().numpy(), want)
        for a, b in zip(planes, y4m.rgb_to_yuv_reference(want, "420", "bt709", False)):
            assert np.array_equal(a.cpu().numpy(), b)


def test_refusals_raise_before_any_launch(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import lib
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    y, u, v = z(2, 6, 10), z(2, 3, 5), z(2, 3, 5)
    sentinel = torch.full((2, 6, 10, 3), 7, dtype=torch.uint8, device=dev)
    wide = z(2, 3, 10)
    bad = [dict(y=y.cpu()), dict(u=u.cpu()), dict(y=y.float()), dict(v=v.int()), dict(y=y[0]), dict(u=z(2, 3, 6)), dict(v=z(2, 4, 5)),
           dict(u=z(3, 3, 5)), dict(u=z(2, 6, 10), v=z(2, 6, 10)),                     # 4:4:4 planes for 4:2:0 luma
           dict(u=None), dict(u=wide[:, :, ::2], v=wide[:, :, ::2]),                   # rows that are not dense
           dict(u=z(2, 6, 5)[:, ::2], v=z(2, 6, 5)[:, ::2]),
           dict(u=z(4, 3, 5)[::2]),                                                    # u and v at different frame strides
           dict(chroma="422"), dict(siting="left"), dict(matrix="bt2020"), dict(chroma="444"),
           dict(out=sentinel[:1]), dict(out=sentinel.float()), dict(out=sentinel.cpu()), dict(out=sentinel.permute(0, 2, 1, 3))]
    for kw in bad:
        a = dict(y=y, u=u, v=v, chroma="420", siting="centre", matrix="bt601", full=False, out=sentinel)
        a.update(kw)
        with pytest.raises(ops.VvaeError):
            ops.yuv_to_rgb_u8(**a)
    rgb = z(2, 6, 10, 3)
    outs = (torch.full((2, 6, 10), 7, dtype=torch.uint8, device=dev), torch.full((2, 3, 5), 7, dtype=torch.uint8, device=dev),
            torch.full((2, 3, 5), 7, dtype=torch.uint8, device=dev))
    for kw in (dict(rgb=rgb.cpu()), dict(rgb=rgb.float()), dict(rgb=rgb[0]), dict(rgb=z(2, 6, 10, 4)), dict(chroma="mono"), dict(chroma="422"),
               dict(matrix="bt2020"), dict(chroma="444"), dict(out=outs[:2]), dict(out=(outs[0], outs[1], outs[2].cpu())),
               dict(out=(outs[0], outs[1], outs[2][:1]))):
        a = dict(rgb=rgb, chroma="420", matrix="bt601", full=False, out=outs)
        a.update(kw)
        with pytest.raises(ops.VvaeError):
            ops.rgb_to_yuv(**a)
    assert ops.yuv_supported(16384, 16384, "mono") and not ops.yuv_supported(16385, 2) and not ops.yuv_supported(2, 0) \
        and not ops.yuv_supported(2, 2, "422")
    # the launcher's own checks
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = lib()
    for args in ((p(y), p(u), p(v), 60, 15, p(sentinel), 0, 6, 10, 0, 0, 0, 0), (p(y), p(u), p(v), 60, 15, p(sentinel), 2, 6, 10, 3, 0, 0, 0),
                 (p(y), p(u), p(v), 60, 15, p(sentinel), 2, 6, 10, 0, 2, 0, 0), (p(y), p(u), p(v), 60, 15, p(sentinel), 2, 6, 10, 0, 0, 2, 0),
                 (p(y), None, p(v), 60, 15, p(sentinel), 2, 6, 10, 0, 0, 0, 0), (None, p(u), p(v), 60, 15, p(sentinel), 2, 6, 10, 0, 0, 0, 0),
                 (p(y), p(u), p(v), -60, 15, p(sentinel), 2, 6, 10, 0, 0, 0, 0), (p(y), p(u), p(v), 60, 15, p(sentinel), 2, 16385, 10, 0, 0, 0, 0)):
        assert L.vvae_yuv_to_rgb_u8(*args, st) == 1001, args
    for args in ((p(rgb), p(outs[0]), p(outs[1]), p(outs[2]), 0, 6, 10, 0, 0, 0), (p(rgb), p(outs[0]), p(outs[1]), p(outs[2]), 2, 6, 10, 2, 0, 0),
                 (p(rgb), p(outs[0]), None, p(outs[2]), 2, 6, 10, 0, 0, 0), (p(rgb), p(outs[0]), p(outs[1]), p(outs[2]), 2, 6, 10, 0, 2, 0)):
        assert L.vvae_rgb_to_yuv(*args, st) == 1001, args
    torch.cuda.synchronize()
    assert (sentinel == 7).all() and all((o == 7).all() for o in outs)


# ------------------------------------------------------------------------------------------------ the clip on the device
def test_fixture_files_convert_on_the_device_to_the_fixture_s_rgb(dev):
    """The four fixture files (FRAME lines of 6 and 9 bytes in one of them: three runs) through data.upload_rgb."""
    from video_vae_amd import data as D
    from video_vae_amd import y4m
    with np.load(os.path.join(GOLDEN, "y4m_small_rgb.npz")) as z:
        want = {k: z[k] for k in z.files}
    for form, name in (("420", "y4m_small.y4m"), ("420mpeg2", "y4m_small_mpeg2.y4m"), ("444", "y4m_small_444.y4m"), ("mono", "y4m_small_mono.y4m")):
        for matrix in ("bt601", "bt709"):
            for rng in ("limited", "full"):
                clip = y4m.Y4MClip(os.path.join(GOLDEN, name), matrix, rng)
                got = D.upload_rgb(clip, dev)
                assert got.is_cuda and np.array_equal(got.cpu().numpy(), want[f"{form}_{matrix}_{rng}"]), (form, matrix, rng)


def test_upload_centre_square_of_a_y4m_clip_equals_the_host_path(dev, tmp_path):
    from video_vae_amd import data as D
    from video_vae_amd import y4m
    from video_vae_amd.infer import centre_square
    rgb = np.random.default_rng(9).integers(0, 256, size=(5, 45, 80, 3), dtype=np.uint8)
    path = str(tmp_path / "c.y4m")
    y4m.write(path, rgb)
    clip = y4m.Y4MClip(path)
    want = centre_square(clip[:], 32)                                                  # host conversion, host crop + resize
    per = clip.header.frame_bytes
    one = D.upload_centre_square(clip, 32, dev, run_bytes=per)                         # runs of one frame
    assert clip.runs(0, 5, per) == [(i, i + 1) for i in range(5)]
    assert one.shape == (5, 32, 32, 3) and np.array_equal(one.cpu().numpy(), want)
    assert torch.equal(D.upload_centre_square(clip, 32, dev), one)                     # one run
    assert torch.equal(D.upload_centre_square(clip, 32, dev, run_bytes=2 * (per + 80)), one)
    assert np.array_equal(D.upload_rgb(clip, dev, run_bytes=per).cpu().numpy(), clip[:])


# ------------------------------------------------------------------------------------------------ command line
SIZE = 32


def _small(seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    return rl_model.VideoVAE(rngs=V.Rngs(seed), **model_config(SIZE, True))


def _run(args):
    """The command in this process (infer.main is what ``python -m video_vae_amd.infer`` calls)."""
    from video_vae_amd import infer
    infer.main([str(a) for a in args])


def _scene(rng, frames, hw, lo, hi):
    """Frames of four flat quadrants in the four colours of one palette drawn from [lo, hi), in a new order in every frame: one histogram
    per scene, also behind the chroma subsampling."""
    pal = rng.integers(lo, hi, size=(4, 3))
    out = np.zeros((frames,) + hw + (3,), dtype=np.uint8)
    for f in range(frames):
        p = pal[rng.permutation(4)]
        out[f, :hw[0] // 2, :hw[1] // 2], out[f, :hw[0] // 2, hw[1] // 2:] = p[0], p[1]
        out[f, hw[0] // 2:, :hw[1] // 2], out[f, hw[0] // 2:, hw[1] // 2:] = p[2], p[3]
    return out


def _data(tmp_path):
    """Two folders of the same clips: .y4m files (one 4:2:0 limited, one 4:4:4 full range), and the .npy of their reference RGB.  45 x 57:
    odd sides; 10 frames in two scenes of distinct colour, and 6 frames."""
    from video_vae_amd import y4m
    rng = np.random.default_rng(4)
    clips = {"wide": (np.concatenate([_scene(rng, 6, (45, 57), 0, 70), _scene(rng, 4, (45, 57), 180, 256)]), "420", False),
             "low": (_scene(rng, 6, (24, 30), 0, 256), "444", True)}
    a, b = tmp_path / "data_y4m", tmp_path / "data_npy"
    a.mkdir()
    b.mkdir()
    for name, (rgb, chroma, full) in clips.items():
        y4m.write(str(a / f"{name}.y4m"), rgb, chroma=chroma, full=full)
        np.save(b / f"{name}.npy", y4m.Y4MClip(str(a / f"{name}.y4m"))[:])
    return a, b


def _common(tmp_path, data):
    return ["--model_path", str(tmp_path / "ckpt"), "--data", str(data), "--size", str(SIZE), "--frames", "4", "--batch", "4", "--small",
            "--threshold"]


@pytest.mark.parametrize("mode", ["device_resize", "scene_cuts"])
def test_cli_encode_of_y4m_clips_writes_the_latents_of_their_rgb(dev, tmp_path, mode):
    from video_vae_amd import model_loader
    a, b = _data(tmp_path)
    model_loader.save_checkpoint(_small(9), None, str(tmp_path / "ckpt"))
    flags = {"device_resize": ["--device-resize"], "scene_cuts": ["--scene-cuts"]}[mode]
    for tag, data in (("y4m", a), ("npy", b)):
        _run(["encode"] + _common(tmp_path, data) + flags + ["--out", str(tmp_path / f"lat_{tag}")])
    for name in ("wide", "low"):
        with np.load(tmp_path / "lat_y4m" / f"{name}.npz") as p, np.load(tmp_path / "lat_npy" / f"{name}.npz") as q:
            assert sorted(p.files) == sorted(q.files)
            for k in p.files:
                assert p[k].dtype == q[k].dtype and p[k].shape == q[k].shape and p[k].tobytes() == q[k].tobytes(), (name, k)
            if mode == "scene_cuts":
                assert p["scene_cuts"].tolist() == ([6] if name == "wide" else [])


def test_cli_scenes_prints_the_same_cuts(dev, tmp_path, capsys):
    a, b = _data(tmp_path)
    res = {}
    for tag, data in (("y4m", a), ("npy", b)):
        _run(["scenes", "--data", data, "--out", tmp_path / f"{tag}.json"])
        res[tag] = json.loads((tmp_path / f"{tag}.json").read_text())["clips"]
        lines = [ln.split(": ", 1)[1] for ln in capsys.readouterr().out.splitlines() if "scenes, cuts at" in ln]
        res[tag + "_lines"] = lines
    assert res["y4m_lines"] == res["npy_lines"] and len(res["y4m_lines"]) == 2
    for p, q in zip(res["y4m"], res["npy"]):
        assert {k: p[k] for k in p if k != "path"} == {k: q[k] for k in q if k != "path"}
    assert [c["cuts"] for c in res["y4m"]] == [[], [6]]                                 # low, wide


def test_cli_decode_ext_y4m_writes_the_bytes_of_the_host_writer(dev, tmp_path):
    from video_vae_amd import model_loader, y4m
    a, _ = _data(tmp_path)
    model_loader.save_checkpoint(_small(9), None, str(tmp_path / "ckpt"))
    _run(["encode"] + _common(tmp_path, a) + ["--out", str(tmp_path / "lat")])
    dec = ["decode", "--model_path", tmp_path / "ckpt", "--latents", tmp_path / "lat", "--batch", "4"]
    _run(dec + ["--out", tmp_path / "npy", "--ext", "npy"])
    _run(dec + ["--out", tmp_path / "y4m", "--ext", "y4m"])
    _run(dec + ["--out", tmp_path / "y4m709", "--ext", "y4m", "--y4m-matrix", "bt709", "--y4m-range", "full", "--y4m-chroma", "444", "--fps",
                "30000:1001"])
    for name, frames in (("wide", 10), ("low", 6)):
        rgb = np.load(tmp_path / "npy" / f"{name}.npy")
        assert rgb.shape == (frames, SIZE, SIZE, 3)
        for out, kw in (("y4m", dict()), ("y4m709", dict(fps=(30000, 1001), chroma="444", matrix="bt709", full=True))):
            y4m.write(str(tmp_path / "want.y4m"), rgb, **kw)
            got = (tmp_path / out / f"{name}.y4m").read_bytes()
            assert got == (tmp_path / "want.y4m").read_bytes(), (name, out)
        clip = y4m.Y4MClip(str(tmp_path / "y4m709" / f"{name}.y4m"), matrix="bt709")
        assert clip.shape == rgb.shape and clip.full and clip.header.fps == (30000, 1001)
        assert np.abs(clip[:].astype(int) - rgb).max() <= 1                            # 4:4:4 full range: within the derived bound
