"""csrc/plane_metrics.hip (ops.plane_metrics_u8, plane_metrics.plane_metrics on GPU tensors) against the float64 / int64 definition of
video_vae_amd/plane_metrics.py: the squared errors at zero tolerance, SSIM-Y within 1e-4 absolute (the bar tests/test_gpu_metrics.py
holds the SSIM kernel to), at every geometry at which the kernel takes another path; views of frame records at every residue mod 4 with
the bytes around the planes poisoned; sums past 2^32; more frames than a grid dimension; capture; refusals; ``infer compare`` and
``infer eval --yuv-metrics`` end to end."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF, TEST = os.path.join(GOLDEN, "plane_metrics_ref.y4m"), os.path.join(GOLDEN, "plane_metrics_test.y4m")
SSIM_TOL = 1e-4
MARGIN = 64
CHROMAS = ("420", "444", "mono")


@functools.lru_cache(maxsize=None)
def _constants():
    """The kernel's constants, read from its source."""
    with open(os.path.join(ROOT, "video_vae_amd", "csrc", "plane_metrics.hip")) as fh:
        return {k: int(v) for k, v in re.findall(r"constexpr int PM_(\w+) = (\d+);", fh.read())}


def _geometries():
    c = _constants()
    one = c["STRIP"] + 10                                              # the widest frame one workgroup spans (one strip)
    two = 2 * c["STRIP"] + 10                                          # the widest frame of two strips
    assert one <= c["SPAN"] and c["MIN_BAND"] == 16
    sizes = [(11, 11), (12, 13), (17, 31), (33, 70), (2 * c["MIN_BAND"] + 3, 40)]
    sizes += [(12, w) for w in (one - 1, one, one + 1, one + 2, c["SPAN"], c["SPAN"] + 1, two - 1, two, two + 1, two + 2)]
    return sizes


def _chroma_shape(h, w, chroma):
    return {"420": ((h + 1) // 2, (w + 1) // 2), "444": (h, w), "mono": (0, 0)}[chroma]


def _make(kind, rng, n, r, c):
    """One plane pair (n, r, c) uint8 of a kind of content."""
    if kind == "random":
        return rng.integers(0, 256, size=(n, r, c), dtype=np.uint8), rng.integers(0, 256, size=(n, r, c), dtype=np.uint8)
    if kind == "ramp":                                                 # a smooth ramp plus +- 2 noise
        yy, xx = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
        base = (20 + 200.0 * (yy + 2 * xx) / max(1, r + 2 * c))[None] + 7 * np.arange(n)[:, None, None]
        noisy = lambda: np.clip(np.rint(base) + rng.integers(-2, 3, size=(n, r, c)), 0, 255).astype(np.uint8)
        return noisy(), noisy()
    if kind == "constant":                                             # constant per plane: zero variance
        a, b = rng.integers(0, 256, size=(2, n, 1, 1), dtype=np.uint8)
        return np.broadcast_to(a, (n, r, c)).copy(), np.broadcast_to(b, (n, r, c)).copy()
    assert kind == "identical"
    a = rng.integers(0, 256, size=(n, r, c), dtype=np.uint8)
    return a, a.copy()


@functools.lru_cache(maxsize=None)
def _case(kind, n, h, w, chroma, seed=0):
    """(ref planes, test planes, the reference's PlaneMetrics) on the host: computed once per case, shared and left unchanged."""
    from video_vae_amd import plane_metrics as PM
    rng = np.random.default_rng([seed, n, h, w, len(kind), len(chroma)])
    ch, cw = _chroma_shape(h, w, chroma)
    ya, yb = _make(kind, rng, n, h, w)
    if chroma == "mono":
        a, b = (ya, None, None), (yb, None, None)
    else:
        (ua, ub), (va, vb) = _make(kind, rng, n, ch, cw), _make(kind, rng, n, ch, cw)
        a, b = (ya, ua, va), (yb, ub, vb)
    for p in a + b:
        if p is not None:
            p.setflags(write=False)
    return a, b, PM.plane_metrics_reference(a, b, chroma)


def _up(planes, dev):
    return tuple(None if p is None else torch.from_numpy(np.array(p)).to(dev) for p in planes)


def _check(dev, kind, n, h, w, chroma):
    from video_vae_amd import ops
    a, b, want = _case(kind, n, h, w, chroma)
    sse, ssim = ops.plane_metrics_u8(_up(a, dev), _up(b, dev), chroma)
    assert sse.dtype == torch.int64 and tuple(sse.shape) == (n, 3) and ssim.dtype == torch.float32 and tuple(ssim.shape) == (n,)
    assert np.array_equal(sse.cpu().numpy(), want.sse), (kind, n, h, w, chroma)
    err = np.abs(ssim.cpu().numpy().astype(np.float64) - want.ssim_y).max()
    print(f"plane_metrics {kind} {n}x{h}x{w} {chroma}: max |ssim_y - ref| = {err:.3e}")
    assert err <= SSIM_TOL, (kind, n, h, w, chroma, err)
    return sse, ssim


@pytest.mark.parametrize("chroma", CHROMAS)
def test_sse_is_exact_and_ssim_y_within_1e_4_at_every_geometry(dev, chroma):
    """11 x 11 up, odd sizes, widths around what one workgroup spans and around two strips (from the kernel's constants), two bands plus
    3 rows; 2 frames each."""
    for h, w in _geometries():
        _check(dev, "random", 2, h, w, chroma)


@pytest.mark.parametrize("kind", ["random", "ramp", "constant", "identical"])
def test_every_kind_of_content(dev, kind):
    c = _constants()
    for h, w, chroma in ((33, 70, "420"), (2 * c["MIN_BAND"] + 3, c["STRIP"] + 11, "444"), (11, 11, "mono")):
        sse, ssim = _check(dev, kind, 3, h, w, chroma)
        if kind == "identical":
            from video_vae_amd import plane_metrics as PM
            a, b, _ = _case(kind, 3, h, w, chroma)
            pm = PM.plane_metrics(_up(a, dev), _up(b, dev), chroma)
            assert (sse == 0).all() and (ssim.double() - 1).abs().max().item() <= SSIM_TOL
            planes = slice(0, 1) if chroma == "mono" else slice(0, 3)
            assert (pm.psnr[:, planes] == 100.0).all() and (pm.psnr_yuv == 100.0).all()


# ------------------------------------------------------------------------------------------------ views of frame records
def _records(planes, line, lead, poison):
    """The planes of one operand laid out as a .y4m file lays its frame records out (a FRAME line of ``line`` bytes, then Y, U, V), behind
    MARGIN + lead bytes and before MARGIN more; every byte that is not a plane's is ``poison`` -> (host buffer, offset of record 0, stride)."""
    y, u, v = planes
    n = y.shape[0]
    parts = [p.reshape(n, -1) for p in planes if p is not None]
    stride = line + sum(p.shape[1] for p in parts)
    buf = np.full(MARGIN + lead + n * stride + MARGIN, poison, dtype=np.uint8)
    body = buf[MARGIN + lead:MARGIN + lead + n * stride].reshape(n, stride)
    body[:, line:] = np.concatenate(parts, axis=1)
    return buf, MARGIN + lead, stride


def _views(buf, start, stride, n, h, w, chroma, line):
    ch, cw = _chroma_shape(h, w, chroma)
    y = buf.as_strided((n, h, w), (stride, w, 1), start + line)
    if chroma == "mono":
        return y, None, None
    return (y, buf.as_strided((n, ch, cw), (stride, cw, 1), start + line + h * w),
            buf.as_strided((n, ch, cw), (stride, cw, 1), start + line + h * w + ch * cw))


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("hw", [(13, 17), (33, 71)])
def test_record_views_at_every_residue_equal_dense_copies_bitwise(dev, hw, chroma):
    """FRAME lines of 6 bytes in one operand and of 9 in the other, odd frame sizes, 8 frames and every lead 0 .. 3: over the frames and
    the leads every plane base of each operand meets every residue mod 4, and the two operands sit at different residues.  The bytes
    between the planes and around the buffers are 0 in one operand and 255 in the other: a byte read outside a plane changes the integer
    result."""
    from video_vae_amd import ops
    n, (h, w) = 8, hw
    a, b, want = _case("random", n, h, w, chroma, seed=3)
    dense = ops.plane_metrics_u8(_up(a, dev), _up(b, dev), chroma)
    assert np.array_equal(dense[0].cpu().numpy(), want.sse)
    seen = [set(), set()]
    for lead_a, lead_b in ((0, 0), (1, 1), (2, 2), (3, 3)):          # bases at (lead + 6) % 4 and (lead + 9) % 4: never the same
        views = []
        for k, (planes, line, lead, poison) in enumerate(((a, 6, lead_a, 0), (b, 9, lead_b, 255))):
            host, start, stride = _records(planes, line, lead, poison)
            buf = torch.from_numpy(host).to(dev)
            v = _views(buf, start, stride, n, h, w, chroma, line)
            views.append(v)
            seen[k] |= {(i, (p.data_ptr() + f * stride) % 4) for i, p in enumerate(v) if p is not None for f in range(n)}
        assert views[0][0].data_ptr() % 4 != views[1][0].data_ptr() % 4
        got = ops.plane_metrics_u8(views[0], views[1], chroma)
        assert torch.equal(got[0], dense[0]), (hw, chroma, lead_a, lead_b)
        assert got[1].cpu().numpy().tobytes() == dense[1].cpu().numpy().tobytes(), (hw, chroma, lead_a, lead_b)
    planes = 1 if chroma == "mono" else 3
    for s in seen:
        assert s == {(i, r) for i in range(planes) for r in range(4)}


# ------------------------------------------------------------------------------------------------ sums past 2^32, many frames
def _flat(dev, h, w, chroma, value):
    ch, cw = _chroma_shape(h, w, chroma)
    y = torch.full((1, h, w), value, dtype=torch.uint8, device=dev)
    if chroma == "mono":
        return y, None, None
    return y, torch.full((1, ch, cw), value, dtype=torch.uint8, device=dev), torch.full((1, ch, cw), value, dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("h,w,chroma", [(1080, 1920, "420"), (4320, 8192, "420")])
def test_all_0_against_all_255_is_exact_past_2_32(dev, h, w, chroma):
    """sse_y = 65025 H W is above 2^32 at 1920 x 1080; one frame of 8192 x 4320 is the most any one thread, band and strip sum here."""
    from video_vae_amd import ops
    sse, ssim = ops.plane_metrics_u8(_flat(dev, h, w, chroma, 0), _flat(dev, h, w, chroma, 255), chroma)
    ch, cw = _chroma_shape(h, w, chroma)
    assert 65025 * h * w > 2 ** 32
    assert sse.cpu().tolist() == [[65025 * h * w, 65025 * ch * cw, 65025 * ch * cw]]
    # constant planes 0 and 1: S = C1 / (1 + C1) at every position
    assert abs(float(ssim[0]) - 1e-4 / (1 + 1e-4)) <= SSIM_TOL


def test_more_frames_than_a_grid_dimension(dev):
    """n = 65 537 frames of 11 x 11 4:2:0; frame f of the test is the reference's plus an offset of its own (f mod 251, clipped), so a
    frame swapped or skipped shows in the integer sums."""
    from video_vae_amd import ops
    from video_vae_amd import plane_metrics as PM
    n, h, w = 65537, 11, 11
    rng = np.random.default_rng(8)
    off = (np.arange(n) % 251).astype(np.int64)[:, None, None]
    a = tuple(rng.integers(0, 256, size=(n, r, c), dtype=np.uint8) for r, c in ((11, 11), (6, 6), (6, 6)))
    b = tuple(np.clip(p.astype(np.int64) + off, 0, 255).astype(np.uint8) for p in a)
    want = PM.plane_metrics_reference(a, b, "420")
    assert len({tuple(r) for r in want.sse[:251].tolist()}) == 251
    sse, ssim = ops.plane_metrics_u8(_up(a, dev), _up(b, dev), "420")
    assert np.array_equal(sse.cpu().numpy(), want.sse)
    assert np.abs(ssim.cpu().numpy().astype(np.float64) - want.ssim_y).max() <= SSIM_TOL


# ------------------------------------------------------------------------------------------------ capture, refusals
def test_a_captured_graph_replays_the_eager_results_bitwise(dev):
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    c = _constants()
    n, h, w = 3, 2 * c["MIN_BAND"] + 3, c["STRIP"] + 11
    a, b, want = _case("ramp", n, h, w, "420")
    ga, gb = _up(a, dev), _up(b, dev)
    first = ops.plane_metrics_u8(ga, gb, "420")
    second = ops.plane_metrics_u8(ga, gb, "420")
    torch.cuda.synchronize()
    assert torch.equal(first[0], second[0]) and first[1].cpu().numpy().tobytes() == second[1].cpu().numpy().tobytes()
    assert np.array_equal(first[0].cpu().numpy(), want.sse)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.plane_metrics_u8(ga, gb, "420")
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ops.plane_metrics_u8(ga, gb, "420")
    census = graph_node_census(graph)
    assert census is None or census.get("memset", 0) == 0, census
    for _ in range(2):
        out[0].fill_(-1)
        out[1].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], first[0]) and out[1].cpu().numpy().tobytes() == first[1].cpu().numpy().tobytes()


def test_refusals_raise_before_any_launch(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import lib
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    good = (z(2, 12, 14), z(2, 6, 7), z(2, 6, 7))
    wide = z(2, 6, 14)
    bad = [((good[0].cpu(), good[1], good[2]), good, "420"), (good, (good[0], good[1].cpu(), good[2]), "420"),     # a CPU tensor
           ((good[0].float(), good[1], good[2]), good, "420"), (good, (good[0], good[1], good[2].int()), "420"),   # another dtype
           (good, (good[0], z(2, 6, 6), z(2, 6, 6)), "420"), (good, (good[0], z(2, 12, 14), z(2, 12, 14)), "420"),  # chroma that does not fit
           (good, (good[0], None, None), "420"),
           (good, (good[0], wide[:, :, ::2], wide[:, :, ::2]), "420"),                                            # rows that are not dense
           ((z(2, 24, 14)[:, ::2], good[1], good[2]), good, "420"),
           (good, (good[0], z(4, 6, 7)[::2], good[2]), "420"),                                                     # u and v at different strides
           (good, (z(2, 12, 15), z(2, 6, 8), z(2, 6, 8)), "420"), (good, (z(3, 12, 14), z(3, 6, 7), z(3, 6, 7)), "420"),   # different shapes
           ((z(1, 10, 14), z(1, 5, 7), z(1, 5, 7)),) * 2 + ("420",), ((z(1, 14, 10), None, None),) * 2 + ("mono",),       # below 11
           ((z(1, 11, 8193), None, None),) * 2 + ("mono",), ((z(1, 8193, 11), None, None),) * 2 + ("mono",),              # above 8192
           (good, good, "422"), ((good[0][0], good[1], good[2]), good, "420")]
    for ref, test, chroma in bad:
        with pytest.raises(ops.VvaeError):
            ops.plane_metrics_u8(ref, test, chroma)
    assert ops.plane_metrics_supported(11, 11) and ops.plane_metrics_supported(8192, 8192, "mono")
    assert not ops.plane_metrics_supported(10, 11) and not ops.plane_metrics_supported(11, 8193) and not ops.plane_metrics_supported(16, 16, "422")
    # the launcher's own checks: the outputs are untouched
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = lib()
    sse = torch.full((2, 3), 7, dtype=torch.int64, device=dev)
    ssim = torch.full((2,), 7.0, dtype=torch.float32, device=dev)
    ws = torch.zeros(int(L.vvae_plane_metrics_ws_bytes(2, 12, 14, 0)) + 8, dtype=torch.uint8, device=dev)
    y, u, v = good
    ok = [p(y), p(u), p(v), 168, 42, p(y), p(u), p(v), 168, 42, p(sse), p(ssim), p(ws), 2, 12, 14, 0]
    for i, val in ((0, None), (1, None), (5, None), (7, None), (3, -168), (9, -42), (10, None), (11, None), (12, None), (13, 0), (14, 10),
                   (15, 8193), (16, 3), (16, -1), (12, ctypes.c_void_p(ws.data_ptr() + 4)), (10, ctypes.c_void_p(sse.data_ptr() + 4))):
        args = list(ok)
        args[i] = val
        assert L.vvae_plane_metrics_u8(*args, st) == 1001, (i, val)
    torch.cuda.synchronize()
    assert (sse == 7).all() and (ssim == 7).all()
    assert L.vvae_plane_metrics_u8(*ok, st) == 0
    torch.cuda.synchronize()
    assert (sse == 0).all() and (ssim.double() - 1).abs().max().item() <= SSIM_TOL


def test_plane_metrics_on_gpu_tensors_against_cpu_tensors(dev):
    from video_vae_amd import plane_metrics as PM
    for chroma in CHROMAS:
        a, b, want = _case("ramp", 3, 33, 70, chroma)
        t = lambda planes: tuple(None if p is None else torch.from_numpy(np.array(p)) for p in planes)
        cpu = PM.plane_metrics(t(a), t(b), chroma)
        gpu = PM.plane_metrics(_up(a, dev), _up(b, dev), chroma)
        assert all(torch.is_tensor(v) and v.is_cuda for v in gpu)
        assert np.array_equal(gpu.sse.cpu().numpy(), cpu.sse) and np.array_equal(gpu.samples.cpu().numpy(), cpu.samples)
        assert gpu.mse.dtype == torch.float64 and gpu.psnr.dtype == torch.float64 and gpu.psnr_yuv.dtype == torch.float64
        for k in ("mse", "psnr", "psnr_yuv"):
            assert np.allclose(getattr(gpu, k).cpu().numpy(), getattr(cpu, k), rtol=1e-12, atol=0), (chroma, k)
        assert np.abs(gpu.ssim_y.cpu().numpy().astype(np.float64) - cpu.ssim_y).max() <= SSIM_TOL
        sg, sc = PM.summarize_planes(gpu), PM.summarize_planes(cpu)
        assert sg["frames"] == sc["frames"] == 3 and abs(sg["psnr_y"] - sc["psnr_y"]) <= 1e-10 and abs(sg["ssim_y"] - sc["ssim_y"]) <= SSIM_TOL


# ------------------------------------------------------------------------------------------------ command line
def _run(args):
    """The command in this process (infer.main is what ``python -m video_vae_amd.infer`` calls)."""
    from video_vae_amd import infer
    infer.main([str(a) for a in args])


def _write_y4m(path, planes, lines):
    y, u, v = planes
    with open(path, "wb") as fh:
        fh.write(f"YUV4MPEG2 W{y.shape[2]} H{y.shape[1]} F25:1 Ip C420jpeg\n".encode())
        for f, line in enumerate(lines):
            fh.write(line + y[f].tobytes() + u[f].tobytes() + v[f].tobytes())


def _compare_json(tmp_path, ref, test, tag, monkeypatch=None):
    out = tmp_path / f"{tag}.json"
    if monkeypatch is not None:
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "is_available", lambda: False)
            _run(["compare", "--ref", ref, "--test", test, "--out", out, "--per-frame"])
    else:
        _run(["compare", "--ref", ref, "--test", test, "--out", out, "--per-frame"])
    with open(out) as fh:
        return json.load(fh)


def test_cli_compare_on_the_gpu_equals_the_cpu_route(dev, tmp_path, monkeypatch):
    """The fixture pair and a pair of 16-frame 64 x 48 files whose FRAME lines differ within a file (several runs, intersected); then a
    file against itself."""
    import shutil
    ref, test = tmp_path / "ref", tmp_path / "test"
    ref.mkdir()
    test.mkdir()
    shutil.copy(REF, ref / "small.y4m")
    shutil.copy(TEST, test / "small.y4m")
    a, b, _ = _case("ramp", 16, 48, 64, "420", seed=5)
    s, l = b"FRAME\n", b"FRAME Ip\n"
    _write_y4m(ref / "runs.y4m", a, [s] * 5 + [l] * 4 + [s] * 7)
    _write_y4m(test / "runs.y4m", b, [l] * 2 + [s] * 9 + [l] * 5)
    gpu = _compare_json(tmp_path, ref, test, "gpu")
    cpu = _compare_json(tmp_path, ref, test, "cpu", monkeypatch)
    assert gpu["config"]["device"] == "gpu" and cpu["config"]["device"] == "host"
    with np.load(os.path.join(GOLDEN, "plane_metrics_small.npz")) as z:
        assert gpu["clips"][1]["name"] == "small" and gpu["clips"][1]["per_frame"]["sse"] == z["sse"].tolist()
    for g, c in zip(gpu["clips"], cpu["clips"]):
        assert {k: g[k] for k in ("name", "frames", "height", "width", "chroma", "route")} == \
            {k: c[k] for k in ("name", "frames", "height", "width", "chroma", "route")}
        assert g["route"] == "planes" and g["per_frame"]["sse"] == c["per_frame"]["sse"]
        assert np.abs(np.array(g["per_frame"]["ssim_y"]) - np.array(c["per_frame"]["ssim_y"])).max() <= SSIM_TOL
        for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "mse_y"):
            assert np.allclose(g["per_frame"][k], c["per_frame"][k], rtol=1e-12, atol=0)
            assert abs(g[k] - c[k]) <= 1e-10 * max(1.0, abs(c[k]))
        assert abs(g["ssim_y"] - c["ssim_y"]) <= SSIM_TOL
    assert gpu["dataset"]["frames"] == 19 and abs(gpu["dataset"]["psnr_y"] - cpu["dataset"]["psnr_y"]) <= 1e-9
    same = _compare_json(tmp_path, ref, ref, "same")
    for clip in same["clips"]:
        assert clip["psnr_y"] == clip["psnr_u"] == clip["psnr_v"] == clip["psnr_yuv"] == 100.0 and abs(clip["ssim_y"] - 1) <= SSIM_TOL
        assert all(row == [0, 0, 0] for row in clip["per_frame"]["sse"])


def test_cli_compare_rgb_route_on_the_gpu(dev, tmp_path):
    """An .npy of the first fixture file's RGB against the second file: both through RGB and ops.rgb_to_yuv."""
    import shutil
    from video_vae_amd import plane_metrics as PM, y4m
    ref, test = tmp_path / "ref", tmp_path / "test"
    ref.mkdir()
    test.mkdir()
    a, b = y4m.Y4MClip(REF), y4m.Y4MClip(TEST)
    np.save(ref / "clip.npy", a[:])
    shutil.copy(TEST, test / "clip.y4m")
    (clip,) = _compare_json(tmp_path, ref, test, "rgb")["clips"]
    want = PM.plane_metrics_reference(y4m.rgb_to_yuv_reference(a[:], "420"), y4m.rgb_to_yuv_reference(b[:], "420"), "420")
    assert clip["route"] == "rgb" and clip["per_frame"]["sse"] == want.sse.tolist()
    assert np.abs(np.array(clip["per_frame"]["ssim_y"]) - want.ssim_y).max() <= SSIM_TOL


SIZE = 32
EVAL_CLIP_KEYS = {"name", "path", "frames", "psnr", "ssim", "mse", "kept_fraction", "per_frame"}
EVAL_DATASET_KEYS = {"clips", "frames", "psnr", "ssim", "mse", "kept_fraction"}
PLANE_KEYS = {"psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "ssim_y", "mse_y"}


def _small(seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    return rl_model.VideoVAE(rngs=V.Rngs(seed), **model_config(SIZE, True))


@pytest.mark.parametrize("chroma", ["420", "444"])
def test_cli_eval_yuv_metrics_equal_the_reference_on_the_uint8_frames(dev, tmp_path, monkeypatch, chroma):
    """eval --yuv-metrics --per-frame with the --small model on 32 x 32 clips (6 and 4 frames in windows of 4: a padded window and a
    short batch): per frame the values of plane_metrics_reference on y4m.rgb_to_yuv_reference of the uint8 source windows and of the uint8
    reconstruction, which is taken from the same evaluate runner as the command hands it on.  Without the flag the command writes the
    keys it wrote before."""
    from video_vae_amd import infer, model_loader, plane_metrics as PM, y4m
    rng = np.random.default_rng(11)
    data = tmp_path / "data"
    data.mkdir()
    yy, xx = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing="ij")
    for name, n in (("a", 6), ("b", 4)):
        base = (8 * yy + 3 * xx)[None, :, :, None] + 20 * np.arange(n)[:, None, None, None] + np.array([0, 40, 90])
        np.save(data / f"{name}.npy", np.clip(base % 256 + rng.integers(-9, 10, size=(n, SIZE, SIZE, 3)), 0, 255).astype(np.uint8))
    model_loader.save_checkpoint(_small(9), None, str(tmp_path / "ckpt"))
    common = ["eval", "--model_path", tmp_path / "ckpt", "--data", data, "--size", SIZE, "--frames", 4, "--batch", 4, "--small",
              "--threshold", "--per-frame"]
    seen = []
    inner = infer._yuv_window_metrics

    def spy(args, grp, real, recon, dev_):
        for i in range(real):
            c = grp[i][2]
            src = grp[i][0] if torch.is_tensor(grp[i][0]) else torch.from_numpy(grp[i][0])
            seen.append((src[:c].cpu().numpy(), (recon[i, :c].float().clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()))
        return inner(args, grp, real, recon, dev_)
    monkeypatch.setattr(infer, "_yuv_window_metrics", spy)
    _run(common + ["--out", tmp_path / "yuv.json", "--yuv-metrics", "--yuv-chroma", chroma, "--y4m-matrix", "bt709"])
    with open(tmp_path / "yuv.json") as fh:
        got = json.load(fh)
    assert {k: got["config"][k] for k in ("yuv_metrics", "yuv_chroma", "yuv_matrix", "yuv_range")} == \
        {"yuv_metrics": True, "yuv_chroma": chroma, "yuv_matrix": "bt709", "yuv_range": "limited"}
    src = np.concatenate([s for s, _ in seen])
    rec = np.concatenate([r for _, r in seen])
    assert src.shape == rec.shape == (10, SIZE, SIZE, 3)
    assert np.array_equal(src[:6], np.load(data / "a.npy")) and np.array_equal(src[6:], np.load(data / "b.npy"))
    want = PM.plane_metrics_reference(y4m.rgb_to_yuv_reference(src, chroma, "bt709"), y4m.rgb_to_yuv_reference(rec, chroma, "bt709"), chroma)
    at = 0
    for clip in got["clips"]:
        n = clip["frames"]
        assert set(clip) == EVAL_CLIP_KEYS | PLANE_KEYS
        pf = clip["per_frame"]
        assert pf["sse"] == want.sse[at:at + n].tolist()
        assert np.abs(np.array(pf["ssim_y"]) - want.ssim_y[at:at + n]).max() <= SSIM_TOL
        for i, k in enumerate(("psnr_y", "psnr_u", "psnr_v")):
            assert np.allclose(pf[k], want.psnr[at:at + n, i], rtol=1e-12, atol=0)
            assert abs(clip[k] - want.psnr[at:at + n, i].mean()) <= 1e-10
        assert np.allclose(pf["psnr_yuv"], want.psnr_yuv[at:at + n], rtol=1e-12, atol=0)
        assert np.allclose(pf["mse_y"], want.mse[at:at + n, 0], rtol=1e-12, atol=0)
        assert abs(clip["ssim_y"] - want.ssim_y[at:at + n].mean()) <= SSIM_TOL
        at += n
    assert set(got["dataset"]) == EVAL_DATASET_KEYS | PLANE_KEYS
    assert abs(got["dataset"]["psnr_y"] - want.psnr[:, 0].mean()) <= 1e-10                 # frame-weighted
    # without the flag: the keys of before, and the same values under them
    _run(common + ["--out", tmp_path / "plain.json"])
    with open(tmp_path / "plain.json") as fh:
        plain = json.load(fh)
    assert not any(k.startswith("yuv") for k in plain["config"]) and set(plain["dataset"]) == EVAL_DATASET_KEYS
    for clip, with_flag in zip(plain["clips"], got["clips"]):
        assert set(clip) == EVAL_CLIP_KEYS and set(clip["per_frame"]) == {"psnr", "ssim", "mse", "selection"}
        assert clip["name"] == with_flag["name"] and clip["frames"] == with_flag["frames"]
        assert all(np.isclose(clip[k], with_flag[k], rtol=1e-6, atol=0) for k in ("psnr", "ssim", "mse", "kept_fraction"))
