"""GPU: the tile gather and blend kernels (csrc/tiles.hip) against their definitions, bitwise determinism and graph replay, the wide-frame
metrics against the float64 definition and against frame_metrics, TiledInference against eager reconstruct + blend_tiles and against
GraphedInference, and ``infer eval|encode|decode --tile`` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_metrics_host import ref_metrics
from test_tiling_host import ref_blend

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 64


def _u8(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev)


def _ref_tiles(frames, grid):
    """The eager conversion of every tile: frames[..., y0:y0+S, x0:x0+S, :].float() / 255 with edge indices clamped."""
    out = []
    for q in range(frames.shape[0] * grid.tiles):
        w, k = divmod(q, grid.tiles)
        y0, x0 = grid.origin(k)
        yi = torch.clamp(torch.arange(y0, y0 + grid.tile, device=frames.device), max=grid.height - 1)
        xi = torch.clamp(torch.arange(x0, x0 + grid.tile, device=frames.device), max=grid.width - 1)
        out.append(frames[w][:, yi][:, :, xi].float() / 255)
    return torch.stack(out)


@pytest.mark.parametrize("shape,s,o", [((2, 3, 100, 150, 3), 64, 16), ((1, 2, 40, 48, 3), 64, 16), ((1, 2, 72, 490, 3), 256, 32),
                                       ((2, 2, 90, 77, 1), 32, 8), ((1, 2, 130, 70, 4), 64, 32)])
def test_gather_bitwise(dev, shape, s, o):
    from video_vae_amd.tiling import TileGrid, gather_tiles
    frames = _u8(shape, sum(shape), dev)
    g = TileGrid(shape[2], shape[3], s, o)
    want = _ref_tiles(frames, g)
    got = gather_tiles(frames, g)
    torch.cuda.synchronize()
    assert got.shape == want.shape and torch.equal(got, want)
    if want.shape[0] >= 3:                            # a sub-range into a larger static buffer
        buf = torch.full((4,) + tuple(want.shape[1:]), -1.0, device=dev)
        gather_tiles(frames, g, 1, 2, out=buf)
        assert torch.equal(buf[:2], want[1:3]) and torch.all(buf[2:] == -1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_blend_vs_definition_deterministic_and_graphed(dev, dtype):
    from video_vae_amd.graph import graph_node_census
    from video_vae_amd.tiling import TileGrid, blend_tiles
    g = TileGrid(40, 490, 256, 32)                     # 3 tiles across, column 240 in all three; H < S
    gen = torch.Generator().manual_seed(5)
    tiles = torch.rand((2 * g.tiles, 2, 256, 256, 3), generator=gen).to(dtype)
    want, den_min = ref_blend(tiles.float().numpy(), g)
    assert den_min > 0
    td = tiles.to(dev)
    a = blend_tiles(td, g)
    b = blend_tiles(td, g)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and a.shape == (2, 2, 40, 490, 3)
    err = np.abs(a.cpu().double().numpy() - want)
    assert (err <= 1e-5 * np.abs(want) + 1e-7).all(), float(err.max())
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        blend_tiles(td, g)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = blend_tiles(td, g)
    census = graph_node_census(graph)
    assert census is None or census.get("memset", 0) == 0, census
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


@pytest.mark.parametrize("shape,s,o", [((1, 3, 100, 150, 3), 64, 16), ((2, 2, 72, 490, 3), 256, 32), ((1, 2, 40, 48, 3), 64, 16)])
def test_gather_then_blend_is_the_frame(dev, shape, s, o):
    from video_vae_amd.tiling import TileGrid, blend_tiles, gather_tiles
    frames = _u8(shape, 7, dev)
    g = TileGrid(shape[2], shape[3], s, o)
    got = blend_tiles(gather_tiles(frames, g), g)
    assert (got - frames.float() / 255).abs().max().item() <= 1e-6
    sq = _u8((2, 3, 64, 64, 3), 8, dev)                 # frame = tile: bitwise
    g1 = TileGrid(64, 64, 64, 16)
    assert torch.equal(blend_tiles(gather_tiles(sq, g1), g1), sq.float() / 255)


def _pair(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    y = x + 0.1 * torch.randn(shape, generator=g)
    mask = (torch.rand(shape[:2], generator=g) > 0.3).float()
    mask[0, 0] = 1
    return x.to(dev), y.to(dev), mask.to(dev)


@pytest.mark.parametrize("shape", [(1, 3, 72, 1000, 3), (1, 2, 720, 1280, 3), (2, 2, 24, 3000, 1), (1, 2, 16, 700, 4)])
def test_wide_metrics_vs_float64_definition(dev, shape):
    from video_vae_amd.metrics import frame_metrics_wide
    x32, y32, mask = _pair(shape, sum(shape), dev)
    for dx, dy in [(torch.float32, torch.float32), (torch.float32, torch.bfloat16)]:
        x, y = x32.to(dx), y32.to(dy)
        fm = frame_metrics_wide(x, y, mask)
        torch.cuda.synchronize()
        mse, psnr, ssim = ref_metrics(x.cpu(), y.cpu(), mask.cpu())
        valid = mask.cpu().numpy() != 0
        for got in fm:
            assert got.shape == shape[:2] and torch.all(got[mask == 0] == 0)
        assert np.abs(fm.ssim.cpu().double().numpy() - ssim)[valid].max() <= 1e-4, (dx, dy)
        assert np.abs(fm.psnr.cpu().double().numpy() - psnr)[valid].max() <= 1e-3, (dx, dy)
        np.testing.assert_allclose(fm.mse.cpu().double().numpy(), mse, rtol=1e-4, atol=1e-9)
        again = frame_metrics_wide(x, y, mask)
        for u, v in zip(fm, again):
            assert torch.equal(u, v)


def test_wide_metrics_equal_frame_metrics_where_it_applies(dev):
    from video_vae_amd.metrics import frame_metrics, frame_metrics_wide
    for shape in [(2, 5, 64, 64, 3), (3, 7, 37, 53, 3), (1, 2, 40, 512, 4)]:
        x, y, mask = _pair(shape, 3, dev)
        for u, v in zip(frame_metrics(x, y, mask), frame_metrics_wide(x, y, mask)):
            assert torch.equal(u, v)


def test_wide_metrics_masked_frames(dev):
    from video_vae_amd.metrics import frame_metrics_wide
    x, y, mask = _pair((2, 3, 40, 1280, 3), 4, dev)
    mask[1] = 0
    a = frame_metrics_wide(x, y, mask)
    x2, y2 = x.clone(), y.clone()
    x2[mask == 0] = float("nan")
    b = frame_metrics_wide(x2, y2, mask)
    for u, v in zip(a, b):
        assert torch.equal(u, v) and torch.all(v[1] == 0) and torch.all(torch.isfinite(v))


def _small(flavour, seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def test_tiled_reconstruct_on_square_frames_equals_graphed(dev):
    from video_vae_amd.infer import GraphedInference, InferenceWeights
    from video_vae_amd.tiling import TileGrid, TiledInference
    m = _small("rl", 3).to(dev)
    w = InferenceWeights(m)
    frames = _u8((2, 4, SMALL, SMALL, 3), 2, dev)
    mask = torch.ones(2, 4, device=dev)
    mask[1, 3] = 0
    ti = TiledInference(m, w, TileGrid(SMALL, SMALL, SMALL, 16), 2, 4, "reconstruct")
    out = ti(frames, mask)
    gi = GraphedInference(m, w, 2, 4, "reconstruct")
    want = gi(frames.float() / 255.0, mask)
    assert torch.equal(out.frames, want.float())


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_tiled_reconstruct_equals_eager_chunks(dev, flavour):
    """100 x 150 frames, S = 64, o = 16 (2 x 3 tiles), three windows, batch 4: chunks straddle windows and the last one is short."""
    from video_vae_amd.infer import InferenceWeights
    from video_vae_amd.tiling import TileGrid, TiledInference, blend_tiles, gather_tiles
    m = _small(flavour, 4).to(dev)
    w = InferenceWeights(m)
    g = TileGrid(100, 150, SMALL, 16)
    n, t, b = 3, 4, 4
    frames = _u8((n, t, 100, 150, 3), 5, dev)
    mask = torch.ones(n, t, device=dev)
    mask[2, 2:] = 0
    out = TiledInference(m, w, g, b, t, "reconstruct")(frames, mask)
    tiles = gather_tiles(frames, g)
    total = n * g.tiles
    recon, sels = [], []
    with torch.no_grad():
        for first in range(0, total, b):
            idx = [min(first + j, total - 1) for j in range(b)]
            x = tiles[idx]
            mk = mask[[q // g.tiles for q in idx]]
            lat = m.encode(x, mk, None, want_log_variance=False)
            r = m.decode(lat.compressed_representation, mk)
            cnt = min(b, total - first)
            recon.append(r[:cnt])
            sels.append(lat.selection[:cnt])
    want = blend_tiles(torch.cat(recon), g)
    assert out.frames.shape == (n, t, 100, 150, 3) and torch.equal(out.frames, want)
    assert out.selection.shape == (n, g.tiles, t) and torch.equal(out.selection, torch.cat(sels).reshape(n, g.tiles, t))
    ev = TiledInference(m, w, g, b, t, "evaluate")(frames, mask)
    assert torch.equal(ev.frames, want)
    from video_vae_amd.metrics import frame_metrics_wide
    for u, v in zip(ev.metrics, frame_metrics_wide(frames.float() / 255.0, want, mask)):
        assert torch.equal(u, v)


def _clips(data, rng):
    data.mkdir()
    np.save(data / "wide.npy", rng.integers(0, 256, size=(9, 100, 150, 3), dtype=np.uint8))
    np.save(data / "small.npy", rng.integers(0, 256, size=(5, 40, 48, 3), dtype=np.uint8))


def test_cli_eval_tiled(dev, tmp_path):
    from video_vae_amd import model_loader
    from video_vae_amd.infer import InferenceWeights, clip_windows_native
    from video_vae_amd.tiling import TileGrid, TiledInference
    _clips(tmp_path / "data", np.random.default_rng(6))
    model = _small("rl", 9)
    model_loader.save_checkpoint(model, None, str(tmp_path / "ckpt"))
    out = tmp_path / "m.json"
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "video_vae_amd.infer", "eval", "--model_path", str(tmp_path / "ckpt"),
           "--data", str(tmp_path / "data"), "--size", str(SMALL), "--frames", "4", "--batch", "4", "--small", "--threshold", "--per-frame",
           "--tile", "--overlap", "16", "--out", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(out.read_text())
    assert res["config"]["tile"] is True and res["config"]["overlap"] == 16 and res["dataset"]["frames"] == 14
    clips = {c["name"]: c for c in res["clips"]}
    m = model.to(dev)
    ti = None
    for name, hw, tiles in (("wide", (100, 150), [2, 3]), ("small", (40, 48), [1, 1])):
        e = clips[name]
        assert (e["height"], e["width"]) == hw and e["tiles"] == tiles
        video, mask, counts = clip_windows_native(str(tmp_path / "data" / f"{name}.npy"), 4)
        g = TileGrid(hw[0], hw[1], SMALL, 16)
        ti = TiledInference(m, InferenceWeights(m), g, 4, 4, "evaluate") if ti is None else ti.with_grid(g)
        o = ti(torch.from_numpy(video).to(dev), torch.from_numpy(mask).to(dev))
        per = {k: [] for k in ("psnr", "ssim", "mse", "selection")}
        sel = o.selection.mean(dim=1)
        for i, c in enumerate(counts):
            for k, v in (("psnr", o.metrics.psnr), ("ssim", o.metrics.ssim), ("mse", o.metrics.mse), ("selection", sel)):
                per[k] += v[i, :c].double().cpu().tolist()
        for k in per:
            assert e["per_frame"][k] == per[k], (name, k)
        assert abs(e["kept_fraction"] - float(np.mean(per["selection"]))) <= 1e-12
        assert abs(e["psnr"] - float(np.mean(per["psnr"]))) <= 1e-9 * max(1.0, abs(e["psnr"]))


def test_cli_encode_decode_tiled(dev, tmp_path):
    import video_vae_amd as V
    from video_vae_amd.infer import InferenceWeights, clip_windows_native
    from video_vae_amd.tiling import TileGrid, TiledInference
    _clips(tmp_path / "data", np.random.default_rng(7))
    model = _small("rl", 9)
    V.save_checkpoint(model, None, str(tmp_path / "ckpt"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--model_path", str(tmp_path / "ckpt"), "--batch", "4"]
    enc = ["timeout", "-k", "10", "240", sys.executable, "-m", "video_vae_amd.infer", "encode", "--data", str(tmp_path / "data"), "--out",
           str(tmp_path / "lat"), "--size", str(SMALL), "--frames", "4", "--small", "--threshold", "--tile", "--overlap", "16"] + common
    r = subprocess.run(enc, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    dec = ["timeout", "-k", "10", "240", sys.executable, "-m", "video_vae_amd.infer", "decode", "--latents", str(tmp_path / "lat"), "--out",
           str(tmp_path / "rec")] + common
    r = subprocess.run(dec, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    m = model.to(dev)
    ti = None
    for name, n, hw in (("wide", 9, (100, 150)), ("small", 5, (40, 48))):
        g = TileGrid(hw[0], hw[1], SMALL, 16)
        with np.load(tmp_path / "lat" / f"{name}.npz") as z:
            assert list(z["tile_grid"]) == [hw[0], hw[1], SMALL, 16, g.ny, g.nx] and z["tile_grid"].dtype == np.int64
            assert z["selection"].shape == (g.tiles, n) and z["selection"].dtype == np.uint8 and int(z["n_frames"]) == n
            assert z["mean"].shape == (int(z["selection"].sum()), 16, 96) and z["mean"].dtype == np.float32
        with np.load(tmp_path / "rec" / f"{name}.npz") as z:
            got = z["frames"]
        assert got.shape == (n,) + hw + (3,) and got.dtype == np.uint8
        video, mask, counts = clip_windows_native(str(tmp_path / "data" / f"{name}.npy"), 4)
        ti = TiledInference(m, InferenceWeights(m), g, 4, 4, "reconstruct") if ti is None else ti.with_grid(g)
        o = ti(torch.from_numpy(video).to(dev), torch.from_numpy(mask).to(dev))
        rec = torch.cat([o.frames[i, :c] for i, c in enumerate(counts)]).cpu().numpy()
        want = (np.clip(rec.astype(np.float32), 0, 1) * 255).astype(np.uint8)
        np.testing.assert_array_equal(got, want)
