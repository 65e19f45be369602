"""GPU: the window blend (csrc/tiles.hip) and the temporal-difference metric (csrc/temporal_metrics.hip) against their float64
definitions, bitwise determinism, range-exact writes and agreement with the tile blend; ClipInference against eager encode / decode +
blend_windows and, on hard cuts, against TiledInference; ``infer eval|encode|decode --temporal-overlap`` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_temporal_host import ref_blend_windows, ref_tmse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 64
BLEND_CASES = [(3, 4, 2, (12, 40, 16, 4), 1), (9, 4, 2, (30, 40, 16, 4), 3), (13, 4, 1, (40, 49, 32, 8), 4), (8, 4, 0, (20, 20, 16, 4), 3)]


def _u8(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev)


def _window_tiles(clip, plan, grid):
    """Every window's tiles (windows, ny nx, F, S, S, C) fp32 of a uint8 GPU clip (zero-padded past its end), by the tile gather."""
    from video_vae_amd.tiling import gather_tiles
    f = plan.frames
    if clip.shape[0] < f:
        clip = torch.cat([clip, clip.new_zeros((f - clip.shape[0],) + tuple(clip.shape[1:]))])
    return torch.stack([gather_tiles(clip[st:st + f][None], grid) for st in plan.starts])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("length,frames,o,g,c", BLEND_CASES)
def test_window_blend_vs_definition_deterministic_range_exact(dev, dtype, length, frames, o, g, c):
    from video_vae_amd.tiling import TileGrid, WindowPlan, blend_windows
    plan, grid = WindowPlan(length, frames, o), TileGrid(*g)
    gen = torch.Generator().manual_seed(length + c)
    tiles = torch.rand((plan.windows, grid.tiles, frames, grid.tile, grid.tile, c), generator=gen).to(dtype)
    want = ref_blend_windows(tiles.float().numpy(), plan, grid)
    td = tiles.to(dev)
    a = blend_windows(td, plan, grid)
    b = blend_windows(td, plan, grid)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and a.shape == (length, grid.height, grid.width, c)
    err = np.abs(a.cpu().double().numpy() - want)
    assert (err <= 1e-5 * np.abs(want) + 1e-7).all(), float(err.max())
    assert torch.equal(a, b)
    # one frame range into a sentinel-filled clip: exactly that range is written
    lo, hi = (1, length - 1) if length > 2 else (1, 2)
    out = torch.full_like(a, -7.0)
    blend_windows(td, plan, grid, lo, hi, out=out)
    assert torch.equal(out[lo:hi], a[lo:hi]) and torch.all(out[:lo] == -7.0) and torch.all(out[hi:] == -7.0)
    # the streaming schedule of ClipInference: a ring of plan.ring() slots, each final range blended once
    r = plan.ring()
    ring = torch.full((r,) + tuple(td.shape[1:]), float("nan"), dtype=dtype, device=dev)
    out = torch.full_like(a, -7.0)
    for w in range(plan.windows):
        ring[w % r] = td[w]
        blend_windows(ring, plan, grid, plan.starts[w] if w else 0, plan.final(w), out=out, ring=r)
    assert torch.equal(out, a)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_single_window_frames_equal_tile_blend(dev, dtype):
    from video_vae_amd import ops
    from video_vae_amd.tiling import TileGrid, WindowPlan, blend_windows
    for length, frames, o, g in ((9, 4, 2, (100, 150, 64, 16)), (8, 4, 0, (40, 490, 256, 32)), (10, 4, 1, (64, 64, 64, 0))):
        plan, grid = WindowPlan(length, frames, o), TileGrid(*g)
        gen = torch.Generator().manual_seed(length)
        td = torch.rand((plan.windows, grid.tiles, frames, grid.tile, grid.tile, 3), generator=gen).to(dtype).to(dev)
        clip = blend_windows(td, plan, grid)
        single = 0
        for f in range(length):
            cov = plan.covering(f)
            if len(cov) == 1:
                w = cov[0]
                ref = ops.tile_blend(td[w], grid)[0, f - plan.starts[w]]
                assert torch.equal(clip[f], ref), (length, frames, o, f)
                single += 1
        assert single >= 2


@pytest.mark.parametrize("length,frames,o,hw,s,so", [(9, 4, 2, (100, 150), 64, 16), (5, 8, 2, (40, 48), 64, 16), (13, 4, 1, (72, 490), 256, 32)])
def test_gather_then_blend_windows_is_the_clip(dev, length, frames, o, hw, s, so):
    from video_vae_amd.tiling import TileGrid, WindowPlan, blend_windows
    plan, grid = WindowPlan(length, frames, o), TileGrid(hw[0], hw[1], s, so)
    clip = _u8((length,) + hw + (3,), length, dev)
    got = blend_windows(_window_tiles(clip, plan, grid), plan, grid)
    assert (got - clip.float() / 255).abs().max().item() <= 1e-6
    plan0, g1 = WindowPlan(8, 4, 0), TileGrid(64, 64, 64, 16)     # hard cuts of frame-sized tiles: bitwise
    sq = _u8((8, 64, 64, 3), 8, dev)
    assert torch.equal(blend_windows(_window_tiles(sq, plan0, g1), plan0, g1), sq.float() / 255)


@pytest.mark.parametrize("shape", [(2, 5, 40, 50, 3), (1, 1, 16, 16, 3), (1, 3, 7, 9, 1), (1, 2, 33, 17, 4), (1, 3, 720, 1280, 3)])
def test_tmse_vs_float64_definition(dev, shape):
    from video_vae_amd.metrics import temporal_mse
    g = torch.Generator().manual_seed(sum(shape))
    x32 = torch.rand(shape, generator=g) * 1.2 - 0.1
    y32 = x32 + 0.1 * torch.randn(shape, generator=g)
    for dx, dy in [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]:
        x, y = x32.to(dx), y32.to(dy)
        got = temporal_mse(x.to(dev), y.to(dev))
        again = temporal_mse(x.to(dev), y.to(dev))
        torch.cuda.synchronize()
        assert got.shape == (shape[0], shape[1] - 1) and got.dtype == torch.float32
        np.testing.assert_allclose(got.cpu().double().numpy(), ref_tmse(x.float().numpy(), y.float().numpy()), rtol=1e-4, atol=1e-9)
        assert torch.equal(got, again)
    odd = x32.to(dev)[..., :1].contiguous(), y32.to(dev)[..., :1].contiguous()          # C = 1, rows not a multiple of 4 values
    np.testing.assert_allclose(temporal_mse(*odd).cpu().double().numpy(), ref_tmse(odd[0].cpu().numpy(), odd[1].cpu().numpy()), rtol=1e-4,
                               atol=1e-9)


def _small(flavour, seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_clip_reconstruct_equals_eager_windows(dev, flavour):
    """9 frames of 100 x 150 in windows of 4 overlapping by 2 (starts 0, 1, 3, 5; frame 3 in three windows), 2 x 3 tiles, batch 4: chunks
    straddle windows and the last one is short.  Then a 3-frame clip (one padded window) on the same runner."""
    from video_vae_amd.infer import InferenceWeights
    from video_vae_amd.metrics import frame_metrics_wide
    from video_vae_amd.tiling import ClipInference, TileGrid, WindowPlan, blend_windows
    m = _small(flavour, 4).to(dev)
    w = InferenceWeights(m)
    g = TileGrid(100, 150, SMALL, 16)
    t, b = 4, 4
    ci = ClipInference(m, w, g, b, t, 2, "reconstruct")
    ev = ClipInference(m, w, g, b, t, 2, "evaluate")
    for length in (9, 3):
        clip = _u8((length, 100, 150, 3), 5 + length, dev)
        plan = WindowPlan(length, t, 2)
        out = ci(clip)
        tiles = _window_tiles(clip, plan, g).reshape((-1, t, SMALL, SMALL, 3))
        mask = torch.from_numpy(plan.mask()).to(dev)
        total = tiles.shape[0]
        recon, sels = [], []
        with torch.no_grad():
            for first in range(0, total, b):
                idx = [min(first + j, total - 1) for j in range(b)]
                mk = mask[[q // g.tiles for q in idx]]
                lat = m.encode(tiles[idx], mk, None, want_log_variance=False)
                r = m.decode(lat.compressed_representation, mk)
                cnt = min(b, total - first)
                recon.append(r[:cnt])
                sels.append(lat.selection[:cnt])
        rec = torch.cat(recon).reshape((plan.windows, g.tiles, t) + tuple(recon[0].shape[2:]))
        want = blend_windows(rec, plan, g)
        assert out.plan == plan and out.frames.shape == (length, 100, 150, 3) and torch.equal(out.frames, want)
        assert out.selection.shape == (plan.windows, g.tiles, t)
        assert torch.equal(out.selection, torch.cat(sels).reshape(plan.windows, g.tiles, t))
        e = ev(clip)
        assert torch.equal(e.frames, want)
        for u, v in zip(e.metrics, frame_metrics_wide(clip.float()[None] / 255.0, want[None], torch.ones(1, length, device=dev))):
            assert torch.equal(u, v)


@pytest.mark.parametrize("tiled", [True, False])
def test_clip_hard_cuts_equal_tiled_inference(dev, tiled):
    """Overlap 0 on a multiple of the window: the same frames, selection and metrics as TiledInference on the hard-cut windows."""
    from video_vae_amd.infer import InferenceWeights
    from video_vae_amd.tiling import ClipInference, TiledInference, TileGrid
    m = _small("rl", 6).to(dev)
    w = InferenceWeights(m)
    hw = (100, 150) if tiled else (SMALL, SMALL)
    g = TileGrid(hw[0], hw[1], SMALL, 16 if tiled else 0)
    clip = _u8((8,) + hw + (3,), 3, dev)
    out = ClipInference(m, w, g, 4, 4, 0, "evaluate")(clip)
    ref = TiledInference(m, w, g, 4, 4, "evaluate")(clip.reshape((2, 4) + hw + (3,)), torch.ones(2, 4, device=dev))
    assert out.plan.starts == [0, 4]
    assert torch.equal(out.frames, ref.frames.reshape(out.frames.shape))
    assert torch.equal(out.selection, ref.selection)
    for u, v in zip(out.metrics, ref.metrics):
        assert torch.equal(u.reshape(-1), v.reshape(-1))


def _run(args):
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "video_vae_amd.infer"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _common(tmp_path, data):
    return ["--model_path", str(tmp_path / "ckpt"), "--data", str(data), "--size", str(SMALL), "--frames", "4", "--batch", "4", "--small",
            "--threshold"]


def _eval(tmp_path, data, name, extra):
    out = tmp_path / f"{name}.json"
    _run(["eval"] + _common(tmp_path, data) + ["--per-frame", "--temporal-metrics", "--out", str(out)] + extra)
    return json.loads(out.read_text())


def test_cli_eval_overlap0_equals_hard_cuts(dev, tmp_path):
    from video_vae_amd import model_loader
    rng = np.random.default_rng(11)
    data = tmp_path / "data"
    data.mkdir()
    np.save(data / "wide.npy", rng.integers(0, 256, size=(8, 100, 150, 3), dtype=np.uint8))
    np.save(data / "small.npy", rng.integers(0, 256, size=(4, 40, 48, 3), dtype=np.uint8))
    model_loader.save_checkpoint(_small("rl", 9), None, str(tmp_path / "ckpt"))
    for tile in ([], ["--tile", "--overlap", "16"]):
        hard = _eval(tmp_path, data, "hard", tile)
        o0 = _eval(tmp_path, data, "o0", tile + ["--temporal-overlap", "0"])
        assert o0["config"]["temporal_overlap"] == 0 and "temporal_overlap" not in hard["config"]
        for a, b in zip(hard["clips"], o0["clips"]):
            assert a["name"] == b["name"] and b["windows"] == a["frames"] // 4 and b["stored_ratio"] == 1.0
            for k in ("psnr", "ssim", "mse", "selection", "tmse"):
                assert a["per_frame"][k] == b["per_frame"][k], (tile, a["name"], k)
            for k in ("psnr", "ssim", "mse", "kept_fraction", "tmse", "tmse_seam", "tmse_inner", "pairs", "seam_pairs"):
                assert a[k] == b[k], (tile, a["name"], k)
        by = {c["name"]: c for c in hard["clips"]}
        assert (by["wide"]["pairs"], by["wide"]["seam_pairs"], by["small"]["seam_pairs"]) == (7, 1, 0) and hard["dataset"]["pairs"] == 10


def _clips(data, rng):
    data.mkdir()
    np.save(data / "wide.npy", rng.integers(0, 256, size=(9, 100, 150, 3), dtype=np.uint8))
    np.save(data / "small.npy", rng.integers(0, 256, size=(5, 40, 48, 3), dtype=np.uint8))


def test_cli_eval_encode_decode_overlap2(dev, tmp_path):
    from video_vae_amd import model_loader
    from video_vae_amd.infer import InferenceWeights, centre_square
    from video_vae_amd.metrics import temporal_mse, temporal_summary
    from video_vae_amd.tiling import ClipInference, TileGrid
    _clips(tmp_path / "data", np.random.default_rng(12))
    model = _small("rl", 9)
    model_loader.save_checkpoint(model, None, str(tmp_path / "ckpt"))
    m = model.to(dev)
    w = InferenceWeights(m)
    for tiled in (True, False):
        tile = ["--tile", "--overlap", "16"] if tiled else []
        res = _eval(tmp_path, tmp_path / "data", "o2", tile + ["--temporal-overlap", "2"])
        assert res["config"]["temporal_overlap"] == 2 and res["dataset"]["frames"] == 14
        lat, rec = tmp_path / f"lat{int(tiled)}", tmp_path / f"rec{int(tiled)}"
        _run(["encode"] + _common(tmp_path, tmp_path / "data") + tile + ["--temporal-overlap", "2", "--out", str(lat)])
        _run(["decode", "--model_path", str(tmp_path / "ckpt"), "--batch", "4", "--latents", str(lat), "--out", str(rec)])
        clips = {c["name"]: c for c in res["clips"]}
        ev = rc = None
        for name, n in (("wide", 9), ("small", 5)):
            raw = np.load(tmp_path / "data" / f"{name}.npy")
            clip = raw if tiled else centre_square(raw, SMALL)
            g = TileGrid(clip.shape[1], clip.shape[2], SMALL, 16) if tiled else TileGrid(SMALL, SMALL, SMALL, 0)
            ev = ClipInference(m, w, g, 4, 4, 2, "evaluate") if ev is None else ev.with_grid(g)
            u8 = torch.from_numpy(clip).to(dev)
            o = ev(u8)
            e = clips[name]
            assert e["frames"] == n and e["windows"] == o.plan.windows and e["stored_ratio"] == o.plan.stored_ratio()
            if tiled:
                assert (e["height"], e["width"], e["tiles"]) == (g.height, g.width, [g.ny, g.nx])
            for k, v in (("psnr", o.metrics.psnr), ("ssim", o.metrics.ssim), ("mse", o.metrics.mse)):
                assert e["per_frame"][k] == v[0].double().cpu().tolist(), (tiled, name, k)
            selw = o.selection.mean(dim=1).double().cpu().numpy()
            kept = np.concatenate([selw[i, :c] for i, c in enumerate(o.plan.counts)]).mean()
            assert abs(e["kept_fraction"] - float(kept)) <= 1e-12
            tm = temporal_mse(u8.float()[None] / 255.0, o.frames[None])[0].double().cpu().numpy()
            assert e["per_frame"]["tmse"] == tm.tolist() and len(tm) == n - 1
            summ = temporal_summary(tm, 4)
            for k in summ:
                assert e[k] == summ[k], (tiled, name, k)
            with np.load(lat / f"{name}.npz") as z:
                assert z["window_starts"].tolist() == o.plan.starts and int(z["temporal_overlap"]) == 2
                assert list(z["tile_grid"]) == list(g.as_array()) and int(z["n_frames"]) == n
                assert z["selection"].shape == (o.plan.windows, g.tiles, 4) and z["selection"].dtype == np.uint8
            with np.load(rec / f"{name}.npz") as z:
                got = z["frames"]
            rc = ClipInference(m, w, g, 4, 4, 2, "reconstruct") if rc is None else rc.with_grid(g)
            want = (np.clip(rc(u8).frames.cpu().numpy(), 0, 1) * 255).astype(np.uint8)
            assert got.shape == (n, g.height, g.width, 3) and got.dtype == np.uint8
            np.testing.assert_array_equal(got, want)
