"""Plane-wise Y'CbCr metrics on the host: video_vae_amd/plane_metrics.py (the definition) against the fixture of
tests/golden/make_plane_metrics_fixture.py, its PSNR rules, shapes and refusals, infer's pairing, parser and ``compare`` command on the CPU,
and the three entries of the C ABI.  No GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF, TEST = os.path.join(GOLDEN, "plane_metrics_ref.y4m"), os.path.join(GOLDEN, "plane_metrics_test.y4m")
ENTRIES = ("vvae_plane_metrics_supported", "vvae_plane_metrics_ws_bytes", "vvae_plane_metrics_u8")


def _fixture():
    from video_vae_amd import y4m
    a, b = y4m.Y4MClip(REF), y4m.Y4MClip(TEST)
    with np.load(os.path.join(GOLDEN, "plane_metrics_small.npz")) as z:
        return a, b, z["sse"], z["ssim_y"]


def _planes(rng, n, h, w, chroma):
    from video_vae_amd import y4m
    ch, cw = y4m.chroma_shape(h, w, chroma)
    y = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    if chroma == "mono":
        return y, None, None
    return y, rng.integers(0, 256, size=(n, ch, cw), dtype=np.uint8), rng.integers(0, 256, size=(n, ch, cw), dtype=np.uint8)


def test_the_fixture_files_have_frame_lines_of_6_and_9_bytes():
    a, b, _, _ = _fixture()
    assert a.shape == b.shape == (3, 13, 17, 3) and a.chroma == b.chroma == "420"
    assert a.lines.tolist() == [6, 6, 6] and b.lines.tolist() == [9, 9, 9]


def test_reference_equals_the_fixture():
    from video_vae_amd import plane_metrics as PM
    a, b, sse, ssim = _fixture()
    pm = PM.plane_metrics_reference(a.planes(0, 3), b.planes(0, 3), "420")
    assert pm.sse.dtype == np.int64 and np.array_equal(pm.sse, sse)
    assert pm.ssim_y.dtype == np.float64 and np.abs(pm.ssim_y - ssim).max() <= 1e-12
    assert pm.samples.tolist() == [13 * 17, 7 * 9, 7 * 9]
    assert np.allclose(pm.mse, sse / pm.samples / 255.0 ** 2, rtol=1e-15, atol=0)
    assert np.allclose(pm.psnr, 10 * np.log10(1 / pm.mse), rtol=1e-14, atol=0)


def test_identical_planes_give_100_db_and_ssim_1():
    from video_vae_amd import plane_metrics as PM
    p = _planes(np.random.default_rng(0), 2, 12, 13, "420")
    pm = PM.plane_metrics(p, p, "420")
    assert (pm.sse == 0).all() and (pm.psnr == 100.0).all() and (pm.psnr_yuv == 100.0).all() and (pm.mse == 0).all()
    assert np.abs(pm.ssim_y - 1).max() <= 1e-12


@pytest.mark.parametrize("chroma,weights", [("420", (4, 1, 1)), ("444", (1, 1, 1))])
def test_psnr_yuv_pools_over_the_samples(chroma, weights):
    from video_vae_amd import plane_metrics as PM
    rng = np.random.default_rng(1)
    a, b = _planes(rng, 3, 16, 24, chroma), _planes(rng, 3, 16, 24, chroma)       # even sides: the weights are exact
    pm = PM.plane_metrics_reference(a, b, chroma)
    w = np.array(weights, dtype=np.float64)
    pooled = (pm.mse * w).sum(axis=1) / w.sum()
    assert np.allclose(pm.psnr_yuv, 10 * np.log10(1 / pooled), rtol=1e-13, atol=0)
    tot = pm.sse.sum(axis=1) / pm.samples.sum() / 255.0 ** 2
    assert np.allclose(pm.psnr_yuv, 10 * np.log10(1 / tot), rtol=1e-15, atol=0)


def test_mono_reports_0_for_its_chroma():
    from video_vae_amd import plane_metrics as PM
    rng = np.random.default_rng(2)
    a, b = _planes(rng, 2, 11, 11, "mono"), _planes(rng, 2, 11, 11, "mono")
    pm = PM.plane_metrics(a, b, "mono")
    assert pm.samples.tolist() == [121, 0, 0]
    assert (pm.sse[:, 1:] == 0).all() and (pm.mse[:, 1:] == 0).all() and (pm.psnr[:, 1:] == 0).all()
    assert np.allclose(pm.psnr_yuv, pm.psnr[:, 0], rtol=1e-15, atol=0)
    s = PM.summarize_planes(pm)
    assert s["psnr_u"] == 0 and s["psnr_v"] == 0 and s["frames"] == 2


def test_odd_sides_round_the_chroma_up():
    from video_vae_amd import plane_metrics as PM
    rng = np.random.default_rng(3)
    a, b = _planes(rng, 1, 13, 15, "420"), _planes(rng, 1, 13, 15, "420")
    assert a[1].shape == (1, 7, 8)
    pm = PM.plane_metrics_reference(a, b, "420")
    assert pm.samples.tolist() == [195, 56, 56]
    for p in range(3):
        assert pm.sse[0, p] == sum((int(x) - int(y)) ** 2 for x, y in zip(a[p].reshape(-1), b[p].reshape(-1)))
    with pytest.raises(ValueError, match="8192"):                      # chroma planes of the rounded-down shape do not fit
        PM.plane_metrics_reference((a[0], a[1][:, :6], a[2][:, :6]), b, "420")


def test_refusals_name_the_limits():
    from video_vae_amd import plane_metrics as PM
    big = lambda *s: np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.uint8), shape=s, strides=(0,) * len(s), writeable=False)
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    good = (z(2, 12, 12), z(2, 6, 6), z(2, 6, 6))
    bad = [((z(1, 10, 12), z(1, 5, 6), z(1, 5, 6)),) * 2 + ("420",),                   # below 11
           ((z(1, 12, 10), None, None),) * 2 + ("mono",),
           ((big(1, 8193, 16), None, None),) * 2 + ("mono",),                           # above 8192: by shape only, nothing allocated
           ((big(1, 16, 8193), big(1, 16, 8193), big(1, 16, 8193)),) * 2 + ("444",),
           (good, (z(2, 12, 13), z(2, 6, 7), z(2, 6, 7)), "420"),                       # mismatched shapes
           (good, (z(3, 12, 12), z(3, 6, 6), z(3, 6, 6)), "420"),
           (good, (good[0], z(2, 12, 12), z(2, 12, 12)), "420"),
           (good, (good[0], None, None), "420"),
           ((good[0].astype(np.float32), good[1], good[2]), good, "420"),               # wrong dtype
           (good, (good[0], good[1].astype(np.int8), good[2]), "420"),
           ((torch.zeros(2, 12, 12), None, None),) * 2 + ("mono",),
           ((z(0, 12, 12), None, None),) * 2 + ("mono",),                               # no frames
           (good, good, "422")]
    for ref, test, chroma in bad:
        for fn in (PM.plane_metrics, PM.plane_metrics_reference):
            with pytest.raises(ValueError, match="11 <= H, W <= 8192"):
                fn(ref, test, chroma)


def test_cpu_tensors_run_the_reference():
    from video_vae_amd import plane_metrics as PM
    rng = np.random.default_rng(5)
    for chroma in ("420", "444", "mono"):
        a, b = _planes(rng, 2, 15, 21, chroma), _planes(rng, 2, 15, 21, chroma)
        want = PM.plane_metrics_reference(a, b, chroma)
        t = lambda p: tuple(None if x is None else torch.from_numpy(x) for x in p)
        got = PM.plane_metrics(t(a), t(b), chroma)
        for x, y in zip(got, want):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        assert PM.summarize_planes(got) == PM.summarize_planes(want)
        assert PM.summarize_planes(got)["psnr_y"] == float(want.psnr[:, 0].mean())


# ------------------------------------------------------------------------------------------------ infer: pairing, parser, compare
def _clip(path, rgb):
    from video_vae_amd import y4m
    if str(path).endswith(".y4m"):
        y4m.write(str(path), rgb)
    else:
        np.save(path, rgb)


def test_pair_clips_pairs_by_stem_and_refuses_what_does_not_match(tmp_path):
    from video_vae_amd.infer import pair_clips
    rng = np.random.default_rng(6)
    rgb = lambda n, h, w: rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _clip(a / "one.y4m", rgb(3, 12, 14))
    _clip(b / "one.npy", rgb(3, 12, 14))
    _clip(a / "two.npy", rgb(2, 16, 16))
    _clip(b / "two.y4m", rgb(2, 16, 16))
    pairs = pair_clips(str(a), str(b))
    assert [(p[0], os.path.basename(p[1]), os.path.basename(p[2]), p[3]) for p in pairs] == \
        [("one", "one.y4m", "one.npy", (3, 12, 14)), ("two", "two.npy", "two.y4m", (2, 16, 16))]
    _clip(a / "three.npy", rgb(2, 16, 16))
    with pytest.raises(SystemExit, match="three"):
        pair_clips(str(a), str(b))
    with pytest.raises(SystemExit, match="three"):
        pair_clips(str(b), str(a))
    _clip(b / "three.npy", rgb(2, 16, 18))
    with pytest.raises(SystemExit, match=r"three.*16x16.*16x18"):
        pair_clips(str(a), str(b))
    _clip(b / "three.npy", rgb(5, 16, 16))
    with pytest.raises(SystemExit, match=r"three.*2 frames.*5"):
        pair_clips(str(a), str(b))


def test_run_pieces_intersects_the_runs_of_both_files(tmp_path):
    from video_vae_amd import y4m
    from video_vae_amd.infer import run_pieces
    h, w, n = 12, 12, 8
    rng = np.random.default_rng(7)

    def write(path, lines):
        with open(path, "wb") as fh:
            fh.write(b"YUV4MPEG2 W12 H12 F25:1 Ip C420jpeg\n")
            for line in lines:
                fh.write(line + rng.integers(0, 256, size=h * w * 3 // 2, dtype=np.uint8).tobytes())
        return y4m.Y4MClip(str(path))
    s, l = b"FRAME\n", b"FRAME Ip\n"
    a = write(tmp_path / "a.y4m", [s, s, s, l, l, s, s, s])
    b = write(tmp_path / "b.y4m", [s, l, l, l, l, l, s, s])
    assert a.runs(0, n) == [(0, 3), (3, 5), (5, 8)] and b.runs(0, n) == [(0, 1), (1, 6), (6, 8)]
    pieces = run_pieces(a, b)
    assert pieces == [(0, 1), (1, 3), (3, 5), (5, 6), (6, 8)]
    for p, q in pieces:                                                # each piece is one run of either file
        a.records(p, q)
        b.records(p, q)


def test_parser_accepts_compare_and_yuv_metrics_and_keeps_the_defaults():
    from video_vae_amd.infer import parse_args
    c = parse_args(["compare", "--ref", "a", "--test", "b"])
    assert (c.cmd, c.out, c.per_frame, c.y4m_matrix, c.y4m_range, c.yuv_chroma) == ("compare", "metrics.json", False, "bt601", "header", "420")
    c = parse_args(["compare", "--ref", "a", "--test", "b", "--out", "o.json", "--per-frame", "--yuv-chroma", "444", "--y4m-matrix", "bt709",
                    "--y4m-range", "full"])
    assert (c.out, c.per_frame, c.y4m_matrix, c.y4m_range, c.yuv_chroma) == ("o.json", True, "bt709", "full", "444")
    base = ["eval", "--model_path", "m", "--data", "d"]
    v = parse_args(base)
    assert v.yuv_metrics is False and v.yuv_chroma == "420" and v.ms_ssim is False and v.y4m_range == "header" and v.out == "metrics.json"
    v = parse_args(base + ["--yuv-metrics", "--yuv-chroma", "444"])
    assert v.yuv_metrics is True and v.yuv_chroma == "444"
    for flags in (["--tile"], ["--temporal-overlap", "2"], ["--scene-cuts"]):
        with pytest.raises(SystemExit) as e:
            parse_args(base + ["--yuv-metrics"] + flags)
        assert e.value.code == 2
        parse_args(base + flags)                                       # without the flag they parse as before
    e = parse_args(["encode", "--model_path", "m", "--data", "d", "--out", "o"])
    assert not hasattr(e, "yuv_metrics") and not hasattr(e, "yuv_chroma")
    d = parse_args(["decode", "--model_path", "m", "--latents", "l", "--out", "o"])
    assert (d.ext, d.y4m_range, d.y4m_chroma) == ("npz", "limited", "420") and not hasattr(d, "yuv_metrics")


def _run(args):
    from video_vae_amd import infer
    infer.main([str(a) for a in args])


@pytest.fixture
def no_gpu(monkeypatch):
    """``compare`` chooses its route by torch.cuda.is_available(): the host reference is what this file tests, on any machine."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_compare_on_the_cpu_takes_the_planes_route_for_two_y4m_files(tmp_path, no_gpu, capsys):
    import shutil
    a, b, sse, ssim = _fixture()
    for d, src in (("ref", REF), ("test", TEST)):
        (tmp_path / d).mkdir()
        shutil.copy(src, tmp_path / d / "clip.y4m")
    out = tmp_path / "m.json"
    _run(["compare", "--ref", tmp_path / "ref", "--test", tmp_path / "test", "--out", out, "--per-frame"])
    with open(out) as fh:
        got = json.load(fh)
    assert sorted(got) == ["clips", "config", "dataset"]
    assert got["config"]["device"] == "host"
    (clip,) = got["clips"]
    assert (clip["name"], clip["frames"], clip["height"], clip["width"], clip["chroma"], clip["route"]) == ("clip", 3, 13, 17, "420", "planes")
    assert clip["per_frame"]["sse"] == sse.tolist()
    assert np.abs(np.array(clip["per_frame"]["ssim_y"]) - ssim).max() <= 1e-12
    samples = np.array([13 * 17, 63, 63])
    psnr = 10 * np.log10(1 / (sse / samples / 255.0 ** 2))
    for i, k in enumerate(("psnr_y", "psnr_u", "psnr_v")):
        assert np.allclose(clip["per_frame"][k], psnr[:, i], rtol=1e-13, atol=0)
        assert abs(clip[k] - psnr[:, i].mean()) <= 1e-12
    pooled = 10 * np.log10(1 / (sse.sum(axis=1) / samples.sum() / 255.0 ** 2))
    assert abs(clip["psnr_yuv"] - pooled.mean()) <= 1e-12 and abs(clip["ssim_y"] - ssim.mean()) <= 1e-12
    assert abs(clip["mse_y"] - (sse[:, 0] / samples[0] / 255.0 ** 2).mean()) <= 1e-15
    for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "ssim_y", "mse_y"):
        assert got["dataset"][k] == clip[k]
    assert got["dataset"]["clips"] == 1 and got["dataset"]["frames"] == 3
    assert "compare: 1 clips, 3 frames" in capsys.readouterr().out
    # without --per-frame: no lists
    _run(["compare", "--ref", tmp_path / "ref", "--test", tmp_path / "test", "--out", out])
    with open(out) as fh:
        assert "per_frame" not in json.load(fh)["clips"][0]


@pytest.mark.parametrize("chroma", ["420", "444"])
def test_compare_on_the_cpu_takes_the_rgb_route_for_an_npy_against_a_y4m(tmp_path, no_gpu, chroma):
    import shutil
    from video_vae_amd import plane_metrics as PM, y4m
    a, b, _, _ = _fixture()
    (tmp_path / "ref").mkdir()
    (tmp_path / "test").mkdir()
    np.save(tmp_path / "ref" / "clip.npy", a[:])
    shutil.copy(TEST, tmp_path / "test" / "clip.y4m")
    out = tmp_path / "m.json"
    _run(["compare", "--ref", tmp_path / "ref", "--test", tmp_path / "test", "--out", out, "--per-frame", "--yuv-chroma", chroma])
    with open(out) as fh:
        (clip,) = json.load(fh)["clips"]
    assert clip["route"] == "rgb" and clip["chroma"] == chroma
    want = PM.plane_metrics_reference(y4m.rgb_to_yuv_reference(a[:], chroma), y4m.rgb_to_yuv_reference(b[:], chroma), chroma)
    assert clip["per_frame"]["sse"] == want.sse.tolist()
    assert clip["per_frame"]["ssim_y"] == want.ssim_y.tolist() and clip["per_frame"]["psnr_y"] == want.psnr[:, 0].tolist()
    assert clip["psnr_yuv"] == float(want.psnr_yuv.mean())


def test_compare_names_a_missing_stem(tmp_path, no_gpu):
    import shutil
    (tmp_path / "ref").mkdir()
    (tmp_path / "test").mkdir()
    shutil.copy(REF, tmp_path / "ref" / "clip.y4m")
    shutil.copy(TEST, tmp_path / "test" / "other.y4m")
    with pytest.raises(SystemExit, match="clip|other"):
        _run(["compare", "--ref", tmp_path / "ref", "--test", tmp_path / "test", "--out", tmp_path / "m.json"])


# ------------------------------------------------------------------------------------------------ the library
def test_header_declares_and_library_exports_the_three_entries():
    from video_vae_amd._lib import LIB_PATH, lib, parse_header
    protos = parse_header()
    for name in ENTRIES:
        assert name in protos, f"{name} is not declared in include/vvae_hip.h"
    assert protos["vvae_plane_metrics_ws_bytes"][0] is ctypes.c_size_t and len(protos["vvae_plane_metrics_u8"][1]) == 18
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(ENTRIES) <= exported
    # the two host-only entries answer without a device
    L = lib()
    assert L.vvae_plane_metrics_supported(11, 11, 0) == 1 and L.vvae_plane_metrics_supported(8192, 8192, 2) == 1
    for h, w, c in ((10, 11, 0), (11, 10, 0), (8193, 11, 0), (11, 8193, 1), (16, 16, 3), (16, 16, -1)):
        assert L.vvae_plane_metrics_supported(h, w, c) == 0 and L.vvae_plane_metrics_ws_bytes(1, h, w, c) == 0
    assert L.vvae_plane_metrics_ws_bytes(0, 16, 16, 0) == 0
    assert L.vvae_plane_metrics_ws_bytes(3, 16, 16, 2) == 3 * 16                    # one band, one strip, no chroma
    assert L.vvae_plane_metrics_ws_bytes(3, 16, 16, 0) == 3 * 16 + 3 * 2 * 8
